/*
 * mbn.h — C-ABI of the MI355X-native MobileNet-V1 hot path.
 *
 * Drop-in boundary for the OpenCL "kernel-by-name + positional args" protocol of
 * the reference (anerisheth19/CNN-MobileNet-V1-implementation-on-AWS-FPGA-using-OpenCL):
 * every layer entry point below keeps the NAME and the LEADING POSITIONAL
 * PARAMETERS of one `__kernel` in the reference's kernel.cl, extended by one
 * trailing `const mbn_layer_ext*` that may be NULL.
 *
 *   reference interface replaced                         entry point here
 *   ---------------------------------------------------  -------------------------
 *   kernel.cl:2-3   __kernel convolute(...)              mbn_convolute
 *   kernel.cl:62    __kernel depthwise(...)              mbn_depthwise
 *   kernel.cl:94    __kernel pointwise(...) (also FC,    mbn_pointwise
 *                   MobileNet.c:2681-2763)
 *   kernel.cl:116   __kernel pool(...)                   mbn_pool
 *   MobileNet.c:145-213  CL platform/ctx/queue/program   mbn_init
 *   MobileNet.c:2809-2831 clRelease*                     mbn_shutdown
 *   MobileNet.c:340-342  clCreateBuffer                  mbn_alloc / mbn_free
 *   MobileNet.c:350-351  clEnqueueWriteBuffer            mbn_upload
 *   MobileNet.c:395      clEnqueueReadBuffer             mbn_download
 *   MobileNet.c:390-391  clWaitForEvents + clFinish      mbn_sync
 *   MobileNet.c:301-305  clGetEventProfilingInfo         mbn_last_kernel_ms
 *   MobileNet.c:31-47    readSquezeNetKernel             readSquezeNetKernel (kept) / mbn_read_text_weights
 *   MobileNet.c:49-57    decode_image                    decode_image (kept) / mbn_read_ppm
 *   MobileNet.c:218-238  RGB de-interleave               mbn_split_rgb
 *   MobileNet.c:2771-2792 softmax + argmax               mbn_softmax_argmax_u8 / mbn_softmax_f32
 *   keras.py:1-8 (role only: Keras .h5 -> host weights)  mbn_h5_open / mbn_h5_get / mbn_weights_from_h5
 *   MobileNet.c:13-26 + per-layer literals (topology)    mbn_plan_build
 *   MobileNet.c:240-2763 (29 hand-unrolled layer blocks) mbn_net_create / mbn_net_forward
 *
 * Conventions:
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary;
 *   - every function returns int: 0 = MBN_OK, <0 = MBN_E*; nothing exits/aborts;
 *   - device memory is addressed by raw device pointers (void*) so a caller may
 *     also pass memory it allocated itself (hipMalloc, a torch tensor's data_ptr);
 *   - layer calls are asynchronous on the context's HIP stream (or ext->stream),
 *     ordered; mbn_sync() waits. One context per GPU; a context is not re-entrant.
 *
 * Two arithmetic modes:
 *   LITERAL (ext == NULL or ext->dtype == MBN_DT_U8): the integer semantics of
 *     kernel.cl — uint8 activations, planar NCHW, int32 filters `[oc][ic][ky][kx]`,
 *     int32 accumulate, ReLU, truncating int->uchar store. Bit-exact vs oracle/.
 *   F32 (ext->dtype == MBN_DT_F32): what BASELINE.json's metric measures — fp32,
 *     NHWC, conv -> per-channel scale/shift (folded BatchNorm) -> ReLU/ReLU6,
 *     TF-"SAME" padding. Tolerances: tests/test_parity_gpu.py.
 *   I8 (ext->dtype == MBN_DT_I8): a quantized network — uint8 NHWC activations with one fp32 scale per layer,
 *     int8 filters with one scale per output channel, exact int32 sums, one fp32 requantization per output.
 *     Normative arithmetic: the "int8 inference mode" block below. Bit-exact vs tests/test_int8_gpu.py.
 */
#ifndef MBN_H
#define MBN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status */
#define MBN_OK            0
#define MBN_EINVAL       -1   /* bad argument (NULL pointer, non-positive size, unsupported combo) */
#define MBN_ENOMEM       -2   /* host or device allocation failed */
#define MBN_EDEVICE      -3   /* HIP runtime error (see mbn_last_device_error) */
#define MBN_EIO          -4   /* file missing / short read */
#define MBN_EFORMAT      -5   /* file is not what it claims (HDF5 / PPM / text weights) */
#define MBN_ENOTFOUND    -6   /* named object not in the .h5 */
#define MBN_ESHAPE       -7   /* dataset shape does not match the layer table */
#define MBN_EUNSUPPORTED -8   /* valid request this build does not implement */
#define MBN_ENODEVICE    -9   /* no HIP device / ordinal out of range */

const char *mbn_strerror(int code);

/* ------------------------------------------------------------- enumerations */
enum { MBN_DT_U8 = 0,   /* LITERAL: uint8 act / int32 filter / int32 acc (kernel.cl) */
       MBN_DT_F32 = 1,  /* fp32 act / fp32 filter / fp32 acc                         */
       MBN_DT_BF16 = 2, /* bf16 act / bf16 pointwise filter / fp32 acc (config 5)    */
       MBN_DT_I8 = 3    /* uint8 act (scaled) / int8 per-channel filter / int32 acc  */ };

enum { MBN_LAYOUT_NCHW_PLANAR = 0,  /* plane c at offset c*rows*cols (kernel.cl:73,107) */
       MBN_LAYOUT_NHWC = 1 };

enum { MBN_ACT_NONE = 0, MBN_ACT_RELU = 1 /* kernel.cl:87-89 */, MBN_ACT_RELU6 = 2 /* Keras */ };

/* LITERAL-mode switches; each reproduces one well-defined behaviour of kernel.cl
 * (SURVEY.md Appendix B). ext == NULL uses the context default (mbn_set_literal_quirks;
 * initial default MBN_QUIRKS_KERNEL_CL = what kernel.cl computes wherever it is in bounds). */
#define MBN_Q_CARRY_SUM      0x1u /* B1: `sum` is not reset between output channels (kernel.cl:10,69,99,121) */
#define MBN_Q_DW_PLANE0      0x2u /* B2: depthwise reads input plane 0 for every channel (kernel.cl:83) */
#define MBN_Q_LITERAL_INDEX  0x4u /* kernel.cl:24,83 index expression verbatim:
                                     in[(ty+i)*G0*stride + (tx+j)*stride] over the WHOLE input buffer
                                     (a column past the row end wraps into the next row, a row past the
                                     plane end lands in the next plane); an index past the end of the input
                                     buffer reads 0 (the reference would read out of bounds there: B4/B5) */
#define MBN_Q_POOL_DIV49     0x8u /* kernel.cl:129 divides by the literal 49 whatever filtersize is */
#define MBN_QUIRKS_NONE      0x0u
#define MBN_QUIRKS_KERNEL_CL (MBN_Q_CARRY_SUM | MBN_Q_DW_PLANE0 | MBN_Q_LITERAL_INDEX | MBN_Q_POOL_DIV49)

/* Trailing extension of every layer call. Zero-initialise, set struct_size = sizeof(mbn_layer_ext). */
typedef struct mbn_layer_ext {
    uint32_t struct_size;
    int32_t  batch;        /* N images; 0 or 1 => one image (the reference processes one: MobileNet.c:215) */
    int32_t  dtype;        /* MBN_DT_* */
    int32_t  layout;       /* MBN_LAYOUT_*; F32 requires NHWC, U8 requires NCHW_PLANAR */
    int32_t  act;          /* MBN_ACT_*; LITERAL ignores it (always ReLU, kernel.cl:87) */
    int32_t  pad_top;      /* F32: rows of zero padding above; -1 = TF "SAME" (computed from in/out size) */
    int32_t  pad_left;     /* F32: same for columns. LITERAL always pads filtersize/2 top/left (kernel.cl:79) */
    int32_t  in_rows;      /* depthwise: input plane size; 0 => rows*stride. convolute: ignored */
    int32_t  in_cols;
    int32_t  cin;          /* convolute F32: input channels of the NHWC image (0 => 3) */
    int32_t  gsize0;       /* LITERAL: NDRange of the emulated launch, x then y (get_global_size); 0 => output size */
    int32_t  gsize1;
    uint32_t quirks;       /* LITERAL: MBN_Q_* bitmask. Honoured only when quirks_valid != 0 */
    int32_t  quirks_valid;
    const void *scale;     /* F32: device ptr, op_size floats, multiplies the conv sum (folded BN); NULL => 1 */
    const void *shift;     /* F32: device ptr, op_size floats, added after scale (folded BN / FC bias); NULL => 0 */
    void    *stream;       /* hipStream_t; NULL => the context's stream */
    int32_t  io_flags;     /* MBN_DT_BF16 only: MBN_IO_* (which side of the call is fp32 instead of bf16) */
    int32_t  dilation;     /* depthwise, F32 / BF16: dilation (atrous rate) D of the filter: tap (ky, kx) reads input row oy*stride + ky*D - pad_top,
                            * column likewise; 0 or 1 = none, negative = MBN_EINVAL. pad_top / pad_left = -1 computes SAME with the effective
                            * window (filtersize - 1) * D + 1 (3x3: 2 D + 1, so stride 1 pads D). LITERAL and I8: D > 1 = MBN_EUNSUPPORTED.
                            * Every other call ignores it */
} mbn_layer_ext;

/* bf16 mode (BASELINE config 5): activations bf16 NHWC in HBM, pointwise/FC filters bf16 [Cout][Cin], everything
 * else (conv1/depthwise filters, scale/shift, accumulation) fp32. */
#define MBN_IO_IN_F32   0x1   /* the input tensor is fp32 (convolute: the normalised image) */
#define MBN_IO_OUT_F32  0x2   /* the output tensor is fp32 (pointwise as FC: the logits) */
#define MBN_IO_FILT_PACKED 0x8 /* pointwise, MBN_DT_BF16: `filter_k` holds the plain [Cout][Cin] bf16 filter FOLLOWED, at byte offset
                                * mbn_packed_filter_offset(Cout, Cin), by its packed image (mbn_pack_filter_bf16): the wide-layer GEMM
                                * (mbn_bf16_pw_wide.hip) loads the filter in matrix-operand order straight into registers */
#define MBN_IO_IN_U8    0x4   /* convolute, fp32/bf16 mode: the input is the raw uint8 HWC image (what decode_image /
                               * mbn_read_ppm produce, MobileNet.c:49-57); the Keras MobileNet preprocessing x/127.5 - 1
                               * is applied at load — SURVEY §8f-2, replaces a separate mbn_normalize_u8_to_f32 pass */

typedef struct mbn_context mbn_context;   /* opaque; one per GPU */

/* ----------------------------------------------------------------- lifecycle */
/* Replaces MobileNet.c:145-213 (platform, device, context, queue with profiling, program build). */
int  mbn_init(int device_ordinal, mbn_context **ctx);
/* Replaces MobileNet.c:2809-2831. Frees every buffer still owned by the context. NULL is a no-op. */
int  mbn_shutdown(mbn_context *ctx);
int  mbn_device_count(int *count);                       /* 0 devices => *count = 0, MBN_OK */
int  mbn_device_name(mbn_context *ctx, char *buf, size_t buflen);
int  mbn_device_cus(mbn_context *ctx, int *count);       /* compute units of the context's GPU (256 on MI355X): the counterpart of
                                                          * CL_DEVICE_MAX_COMPUTE_UNITS; the net runner sizes its small-batch choices by it.
                                                          * After mbn_set_planning_cus it is the PLANNING count, so a net created
                                                          * afterwards plans with that */
/* Plan every launch of this context for `cus` compute units instead of the device's own count: persistent grids, the per-XCD tile
 * distributions and the count-dependent kernel choices all size themselves by it. 1 <= cus <= the device's count; 0 restores the
 * device's count; anything else, or a NULL context, is MBN_EINVAL (a grid larger than the device offers nothing). A smaller
 * persistent grid is always legal (no kernel waits on another workgroup) and every kernel's result is the same bits at every count.
 * For tests (the tile loops' multi-round paths are reached by small shapes at small counts) and for a caller that shares the device
 * with other work. It costs a launch nothing. Do not change it while launches of this context are in flight or while a graph is
 * being captured; a net (mbn_net_create) keeps the count it was created under. */
int  mbn_set_planning_cus(mbn_context *ctx, int cus);
int  mbn_device_pci_bus_id(mbn_context *ctx, char *buf, size_t buflen);   /* "0000:05:00.0": which physical GPU this context holds. The
                                                          * reference picks device 0 of platform 0 (MobileNet.c:155); with one context
                                                          * per rank the multi-GPU bench line proves its ranks held N cards */
const char *mbn_last_device_error(mbn_context *ctx);     /* text of the last HIP error seen by this context */
int  mbn_set_literal_quirks(mbn_context *ctx, uint32_t quirks);
int  mbn_get_stream(mbn_context *ctx, void **stream);    /* the context's hipStream_t */
/* Extra streams of the context's device, for overlapping independent work (ext->stream selects one per call).
 * mbn_stream_wait(ctx, waiter, signaler): everything queued on `waiter` after this call runs after everything queued on
 * `signaler` before it (an event record + stream wait, no host sync); NULL names the context's own stream. */
int  mbn_stream_create(mbn_context *ctx, void **stream);
int  mbn_stream_destroy(mbn_context *ctx, void *stream);
int  mbn_stream_wait(mbn_context *ctx, void *waiter, void *signaler);
/* hipGraph capture of a sequence of layer calls (launch-bound small-batch loops): everything queued on `stream`
 * (NULL = the context's stream) between begin and end is recorded instead of executed; mbn_graph_launch replays it as
 * one submission. Blocking calls (mbn_upload/download/sync/alloc/free) must not be made on that stream while capturing;
 * the per-call profiling events are skipped inside a capture. */
int  mbn_graph_begin(mbn_context *ctx, void *stream);
int  mbn_graph_end(mbn_context *ctx, void *stream, void **graph_exec);
int  mbn_graph_launch(mbn_context *ctx, void *graph_exec, void *stream);
int  mbn_graph_destroy(mbn_context *ctx, void *graph_exec);

/* ---------------------------------------------------- buffers (clCreateBuffer &c.) */
/* Every buffer handed out by mbn_alloc is remembered with its size. When a pointer passed to a layer call, a fused call,
 * the classifier calls or mbn_upload/download/memset lies inside one of them (interior pointers included), the bytes the
 * call will touch — computed from its shape arguments, ext->batch and dtype — must fit in the rest of that buffer;
 * otherwise the call returns MBN_EINVAL and launches nothing (mbn_last_device_error names the operand). A uint8 image
 * handed to the fp32 first layer, a logits buffer sized for a smaller batch, a filter shorter than op_size x filtersize
 * are caller errors here, not GPU memory faults. Memory the caller allocated itself is not tracked and not checked. */
int  mbn_alloc(mbn_context *ctx, size_t bytes, void **dptr);                 /* MobileNet.c:340-342 */
int  mbn_free(mbn_context *ctx, void *dptr);
int  mbn_upload(mbn_context *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* blocking, :350 */
int  mbn_download(mbn_context *ctx, void *dst_host, const void *src_dev, size_t bytes); /* blocking, :395 */
int  mbn_memset(mbn_context *ctx, void *dst_dev, int byte, size_t bytes);    /* async on ctx stream */
/* Tell the library that `bytes` of device memory at `dptr` which the CALLER owns are about to be freed or were rewritten
 * behind its back: every library-owned image derived from that range (the pre-split filter images of the opt-in pw_emul
 * form) is released after the device has gone idle. mbn_free does the same for the buffers it hands out; mbn_net_destroy
 * calls this for a caller-provided parameter blob. */
int  mbn_forget(mbn_context *ctx, const void *dptr, size_t bytes);
int  mbn_sync(mbn_context *ctx);                                             /* :390-391 */
/* Time of the most recent layer call in milliseconds (hipEvent pair recorded around its launch on the
 * stream it ran on; waits for it). Replaces clGetEventProfilingInfo START/END (MobileNet.c:301-305). */
int  mbn_last_kernel_ms(mbn_context *ctx, float *ms);
int  mbn_set_profiling(mbn_context *ctx, int enabled);   /* default 0: no events recorded */
/* Event pool for measuring every layer call of a timed region without synchronising inside it:
 * after mbn_profile_begin each layer call records a hipEvent pair on the stream it is launched on into the
 * next free slot (calls beyond `capacity` are not recorded); mbn_profile_end waits for the stream and returns
 * the per-call milliseconds in call order. */
int  mbn_profile_begin(mbn_context *ctx, int capacity);
int  mbn_profile_end(mbn_context *ctx, float *ms, int ms_capacity, int *count);
int  mbn_profile_pause(mbn_context *ctx, int paused);   /* 1: stop recording (slots keep their order), 0: resume */
/* Calibration of the pool: records one event pair exactly as a layer call does, around nothing (with_kernel = 0) or around
 * an empty one-wave kernel (with_kernel = 1), on `stream` (NULL = the context's stream). What such a pair reads is what
 * the pair itself adds to every recorded call (bench.py reports it as `event_overhead_us` and subtracts it, so that short
 * kernels agree with a rocprofv3 kernel trace). */
int  mbn_profile_null(mbn_context *ctx, int with_kernel, void *stream);
/* Step markers: mbn_mark queues one timing event on `stream` (NULL = the context's stream) without synchronising;
 * mbn_marks_read waits for the last one and returns the milliseconds between consecutive marks, in order
 * (count = marks - 1), then forgets them. bench.py brackets every timed step with one mark to report the median and
 * the p10/p90 of the per-step time next to the wall-clock figure. */
int  mbn_mark(mbn_context *ctx, void *stream);
int  mbn_marks_read(mbn_context *ctx, float *ms_between, int capacity, int *count);

/* --------------------------------------------------------------- pointer alignment (tests/test_alignment_gpu.py pins the layer calls and one refusal of every call below;
 * mbn_classifier_tail_fused, the _ex / _u8 stem forms and the uint8 stem image are stated from the code, not tested there)
 * The four layer calls — mbn_convolute, mbn_depthwise, mbn_pointwise, mbn_pool — in F32 and BF16 accept ANY pointer that is a multiple
 * of its own element size (fp32 4 bytes, bf16 2, the MBN_IO_IN_U8 image 1; scale / shift 4) for every operand: an interior pointer of an
 * mbn_alloc buffer, a sliced torch tensor. They never refuse one and never touch a byte outside the tensors. An input, filter or (outside
 * mbn_pointwise) output, scale or shift that is not on 16 bytes (bf16 activations of mbn_depthwise: 8) makes the call take a slower kernel,
 * down to one lane per output element, whose summation order may differ from the aligned call's in the last bits (within the mode's
 * tolerance). mbn_pointwise keeps its GEMM for any element-aligned `out`, `scale` and `shift` (its bf16 epilogue relies on the device's
 * unaligned-access mode for that: mbn_f32_pw.hip); only the bf16 streaming kernels want `out` on 4 and scale / shift on 8 bytes and hand
 * the call to that GEMM otherwise. (I8: 8 bytes, see below; LITERAL is byte-granular.)
 * The other device calls load and store 16 bytes at a time and REFUSE instead, launching nothing:
 *   mbn_dwpw_fused, mbn_dwpw_fused_bf16, mbn_blocks_resident_bf16   any pointer off 16 bytes: MBN_EUNSUPPORTED
 *   mbn_tail_resident_bf16        `in` or a parameter off 16 bytes: MBN_EUNSUPPORTED (`out` is stored per bf16 element: any multiple of 2)
 *   mbn_stem_fused_hw (_ex, _u8)  a filter / scale / shift off 16 bytes: MBN_EUNSUPPORTED; `out` off 16 bytes, an fp32 image off 8 or a
 *                                 uint8 image off 2: MBN_EINVAL
 *   mbn_pool_fc, mbn_classifier_tail_fused   `fc_w` or `workspace` off 16 bytes: MBN_EUNSUPPORTED (`in`, `logits`, `fc_bias`: any multiple of 4)
 *   mbn_convert_f32_to_bf16       `src_f32` off 16 bytes or `dst_bf16` off 8: MBN_EINVAL (mbn_convert_bf16_to_f32: any element-aligned pointer)
 *   mbn_normalize_u8_to_f32       `out_f32` off 16 bytes or `in_u8` off 4: MBN_EINVAL
 * MBN_EUNSUPPORTED is the code a caller answers by issuing the separate layer calls (mbn_net_forward does); MBN_EINVAL has no such fall-back.
 */

/* --------------------------------------------------------------- layer calls
 * Positional parameters are kernel.cl's, in kernel.cl's order and meaning:
 *
 * convolute (kernel.cl:2-3): first 3x3xCin conv.
 *   rows, cols  = INPUT plane size (224); output plane = (rows/stride) x (cols/stride)
 *                 (kernel.cl:14 hard-codes rows/2 * cols/2 as the output plane stride;
 *                 F32 uses ceil division)
 *   LITERAL: inp_r/g/b three uint8 planes; filter int32 [op_size][3][ky][kx]
 *   F32    : inp_r = NHWC image [N][rows][cols][cin]; inp_g/inp_b ignored;
 *            filter fp32 [ky][kx][cin][op_size] (Keras HWIO)
 */
int mbn_convolute(mbn_context *ctx, void *output, const void *inp_image_r, const void *inp_image_g,
                  const void *inp_image_b, const void *filter_k, int rows, int cols, int filtersize,
                  int stride, int op_size, const mbn_layer_ext *ext);

/* depthwise (kernel.cl:62): per-channel 3x3, stride 1 or 2; F32 / BF16: dilated by ext->dilation (output-stride 16 / 8 plans).
 *   rows, cols = OUTPUT plane size (the only use kernel.cl makes of them: output_shift, :73);
 *                input plane = ext->in_rows x in_cols, default rows*stride x cols*stride
 *   op_size    = channels
 *   LITERAL: filter int32 [op_size][ky][kx];  F32: filter fp32 [ky][kx][op_size]
 */
int mbn_depthwise(mbn_context *ctx, void *output, const void *inp_image, const void *filter_k,
                  int rows, int cols, int filtersize, int stride, int op_size, const mbn_layer_ext *ext);

/* pointwise (kernel.cl:94): 1x1 conv = per-pixel [op_size x filtersize] mat-vec; FC when rows=cols=1.
 *   filtersize = number of INPUT channels (loop bound kernel.cl:106, plane stride :107)
 *   filter     = [op_size][filtersize] in both modes (int32 / fp32)
 *   F32 summation order over the input channels: sequential (pw_gemm) for every call of 5 images and more; a call of
 *   ext->batch <= 4 images of a layer with few output tiles (its 4-image form has fewer 64x64 tiles than half the compute
 *   units; K >= 128, K % 64 == 0) runs the split-K kernel: K in 4 / 8 / 16 slices (by K alone) summed in fixed order.
 *   Either way a result depends on the layer and on "1..4 images or more", never on the batch-mates or the slot.
 */
int mbn_pointwise(mbn_context *ctx, void *output, const void *inp_image, const void *filter_k,
                  int rows, int cols, int filtersize, int op_size, const mbn_layer_ext *ext);

/* pool (kernel.cl:116): global filtersize x filtersize average per channel -> [op_size].
 *   rows, cols = input plane size. F32, BF16 and I8: the window is min(filtersize, rows) x min(filtersize, cols), clamped per side,
 *   so filtersize = max(rows, cols) averages the whole plane of a non-square map (what the net runner passes). LITERAL: integer
 *   division (by 49 under MBN_Q_POOL_DIV49).
 */
int mbn_pool(mbn_context *ctx, void *output, const void *inp_image, int rows, int cols, int filtersize,
             int op_size, const mbn_layer_ext *ext);

/* Fused stem (SURVEY §8f-1 applied to the first block): layers 1-3 of the sequence — convolute 3x3x3 stride 2 ->
 * depthwise 3x3 stride 1 -> pointwise 1x1, each followed by its folded-BN scale/shift and ReLU6 — in one kernel, so
 * the two 112x112x32 intermediates never reach HBM (MobileNet.c:240-498 does three launches and six PCIe copies).
 * fp32 NHWC only; image [batch][res][res][3], out [batch][res/2][res/2][c3]; filters in the layouts of the separate
 * calls (w1 [3][3][3][c1], wd [3][3][c1], wp [c3][c1]). Returns MBN_EUNSUPPORTED unless (c1, c3) = (32, 64) (alpha = 1) or
 * (16, 32) (alpha = 0.5) and res is a multiple of 32 — callers then issue the three layer calls instead.
 * mbn_stem_fused, _u8 and _ex are mbn_stem_fused_hw with rows = cols = res. */
int mbn_stem_fused(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                   const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                   int batch, int res, int c1, int c3, void *stream);
/* The same with the raw uint8 HWC image [batch][res][res][3] as input: x/127.5 - 1 is applied while the
 * input patch is loaded, bit-identical to mbn_normalize_u8_to_f32 followed by mbn_stem_fused. */
int mbn_stem_fused_u8(mbn_context *ctx, void *out, const void *image_u8, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int res, int c1, int c3, void *stream);

/* General form: flags = MBN_STEM_IN_U8 (image is raw uint8 HWC) | MBN_STEM_BF16 (the network's bf16 mode, BASELINE
 * config 5: `out` is bf16, `wp` is the bf16 copy of the pointwise filter, both on-chip intermediates are rounded to bf16
 * where the separate launches would store them; everything else — image unless IN_U8, the other filters, scale/shift,
 * arithmetic — stays fp32). */
#define MBN_STEM_IN_U8  0x1
#define MBN_STEM_BF16   0x2
int mbn_stem_fused_ex(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int res, int c1, int c3, int flags, void *stream);
/* rows x cols images: image [batch][rows][cols][3] (fp32, or uint8 with MBN_STEM_IN_U8), out [batch][rows/2][cols/2][c3]; both sides
 * multiples of 32, otherwise as mbn_stem_fused_ex (MBN_EUNSUPPORTED outside the envelope). */
int mbn_stem_fused_hw(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int rows, int cols, int c1, int c3, int flags, void *stream);

/* Fused block: a depthwise 3x3 (stride 1 or 2) + pointwise 1x1 pair of the sequence (the pairs L4-5 ...
 * L26-27, MobileNet.c:322-2599; kernel.cl:62-92 + 94-114) in one kernel, each stage followed by its folded-BN
 * scale/shift and ReLU6; the depthwise output never reaches HBM. fp32 NHWC: in [batch][in_rows][in_cols][cin],
 * out [batch][out_rows][out_cols][cout]; wd [3][3][cin], wp [cout][cin] as in the separate calls; pad_top/pad_left as in
 * mbn_layer_ext (zero padding; the high side needs none stated). Bit-identical to mbn_depthwise followed by
 * mbn_pointwise. Returns MBN_EUNSUPPORTED unless cin is a multiple of 32 and <= 1024, cout a multiple of 128 and <= 1024, out_cols
 * even and the input under 3.75 GiB — callers then issue the two layer calls instead. Three kernels sit behind it, all with the same bits
 * (round 6: stride 1 with cin 128 / 256 runs on the wave-private form mbn_f32_dwpw3.hip, everything else on mbn_f32_dwpw2.hip / mbn_f32_dwpw.hip). */
int mbn_dwpw_fused(mbn_context *ctx, void *out, const void *in, const void *wd, const void *s2, const void *b2,
                   const void *wp, const void *s3, const void *b3, int batch, int in_rows, int in_cols, int out_rows,
                   int out_cols, int cin, int cout, int stride, int pad_top, int pad_left, void *stream);

/* A RUN of equal fused blocks with the activations resident on chip (round 6; bf16 mode): `nblocks` consecutive depthwise 3x3 (stride 1, zero
 * padding 1) + pointwise 1x1 pairs of the sequence (MobileNet.c:322-2599; kernel.cl:62-92 + 94-114) with `channels` channels in and out on a
 * rows x cols map, each stage followed by its folded-BN scale/shift and ReLU6, in ONE launch: an image's map stays in LDS from the first block's input to
 * the last block's output, only the filters come from memory. in / out: bf16 NHWC [batch][rows][cols][channels]; per block: wd [3][3][channels],
 * s2, b2 [channels] fp32, wp_bf16 [channels][channels] bf16, s3, b3 [channels] fp32, as in mbn_dwpw_fused_bf16. Same arithmetic as the separate bf16
 * launches within the bf16 tolerance. Returns MBN_EUNSUPPORTED unless channels == 256, rows * cols <= 104, (rows + 2) * (cols + 2) <= 144 and
 * 1 <= nblocks <= 8 (the five 256 -> 256 blocks on the 10 x 10 map of the 0.5x160 network) — callers then issue the blocks one by one. */
typedef struct mbn_block_params {
    const void *wd, *s2, *b2;       /* depthwise filter, scale, shift (fp32) */
    const void *wp_bf16;            /* pointwise filter [cout][cin], bf16 */
    const void *s3, *b3;            /* pointwise scale, shift (fp32) */
} mbn_block_params;
int mbn_blocks_resident_bf16(mbn_context *ctx, void *out, const void *in, const mbn_block_params *blocks, int nblocks, int batch,
                             int rows, int cols, int channels, void *stream);

/* The network's last two blocks and the global average pool in ONE launch with an image's maps resident on chip (round 6; bf16 mode): depthwise 3x3
 * stride 2 on c0 channels -> pointwise c0 -> c1 -> depthwise 3x3 stride 1 -> pointwise c1 -> c1 -> average over the whole map (layers 24-28 of the
 * sequence: MobileNet.c:322-2599 pairs + the `pool` launch :2601-2679; kernel.cl:62-92, 94-114, 116-132), every stage with its folded-BN scale / shift
 * and ReLU6 and rounded to bf16 as the separate launches store it. in: bf16 NHWC [batch][rows][cols][c0]; out: bf16 [batch][c1] (what mbn_pool writes:
 * the FC layer's input); blocks[0] / blocks[1]: the parameters of the two blocks as in mbn_dwpw_fused_bf16 (blocks[0].wp_bf16 is [c1][c0]).
 * Same arithmetic as the five separate bf16 launches within the bf16 tolerance (depthwise sums and the pool's sum bit for bit; the pointwise sums
 * group their products by 16 instead of 32). Returns MBN_EUNSUPPORTED unless c0 == 256, c1 == 512 and rows, cols are even and <= 10 (the 0.5x160
 * network: 10 x 10 x 256 -> 5 x 5 x 512 -> 512) — callers then issue the layers one by one. */
int mbn_tail_resident_bf16(mbn_context *ctx, void *out, const void *in, const mbn_block_params *blocks, int batch, int rows, int cols, int c0, int c1,
                           void *stream);

/* Classifier tail on device, fp32 (replaces the host loop MobileNet.c:2771-2792):
 * probs[n][k] = softmax(logits[n][:]) and argmax[n] (0-based). probs or argmax may be NULL. */
int mbn_softmax_f32(mbn_context *ctx, void *probs, void *argmax_i32, const void *logits, int batch,
                    int classes, void *stream);

/* The same block in the network's bf16 mode (BASELINE config 5): in/out are bf16 NHWC, wp_bf16 is the bf16 copy of the
 * pointwise filter [cout][cin]; the depthwise filter and all scale/shift vectors stay fp32, arithmetic is fp32, the
 * depthwise output is rounded to bf16 where the separate launch would store it. cin must be a multiple of 64 or 32 itself (half a chunk, padded), cout a multiple
 * of 64 (round 5; a 64-column remainder — block 6-7 of the 0.5x network: 64 -> 64 channels — runs on a 128-column tile whose
 * upper half multiplies zeros and stores nothing). */
int mbn_dwpw_fused_bf16(mbn_context *ctx, void *out, const void *in, const void *wd, const void *s2, const void *b2,
                        const void *wp_bf16, const void *s3, const void *b3, int batch, int in_rows, int in_cols, int out_rows,
                        int out_cols, int cin, int cout, int stride, int pad_top, int pad_left, void *stream);

/* softmax + top-k on device: for every image the k <= 8 most probable classes, most probable first
 * (ties -> lowest index), topk_idx [batch][k] int32 (0-based, -1 when classes < k) and topk_prob [batch][k] fp32;
 * probs (may be NULL) additionally receives the full [batch][classes] distribution. Only 2k values per image have to
 * cross PCIe instead of the 1000 logits of MobileNet.c:2744 + the host exp loop :2771-2792. */
int mbn_softmax_topk_f32(mbn_context *ctx, void *probs, void *topk_idx_i32, void *topk_prob_f32, const void *logits,
                         int batch, int classes, int k, void *stream);
/* Dense head read-out (segmentation; the reference has none: its only read-out is MobileNet.c:2771-2792 over 1000 pooled logits): bilinear upsample of
 * per-pixel logits by `factor` and the argmax over the classes, in one kernel that never writes the upsampled tensor (mbn_f32_dense.hip).
 * logits: fp32 NHWC [batch][rows][cols][classes]; labels_i32: [batch][rows*factor][cols*factor] int32; score_f32 (may be NULL): the same shape in
 * fp32, the winning interpolated logit. factor 8, 16 or 32, an image's logits and an image's output map each below 2^31 bytes, batch <= 65535:
 * otherwise MBN_EUNSUPPORTED. NULL labels / logits, a non-positive size or a pointer off 4 bytes: MBN_EINVAL. Any 4-byte-aligned pointer is taken
 * (`logits` on 16 bytes with classes % 4 == 0 loads 16 bytes at a time; same results).
 * The arithmetic, normative (tests/dense_ref.py reproduces it bit for bit in numpy float32). Half-pixel centres, as
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False). For output row oy, with S = factor:
 *     num = max(2*oy + 1 - S, 0);  y0 = num / (2S) (integer division);  y1 = min(y0 + 1, rows - 1);
 *     fy = (float)(num % (2S)) / (float)(2S);  wy1 = fy;  wy0 = 1.0f - fy
 * and x0, x1, wx0, wx1 from the output column ox and `cols` likewise. Every weight is an exact dyadic fraction, so only the three sums below round.
 * Per class c, without FMA contraction (fmul / fadd each round to nearest even):
 *     t0 = fadd(fmul(x[y0][x0][c], wx0), fmul(x[y0][x1][c], wx1))        horizontal first
 *     t1 = fadd(fmul(x[y1][x0][c], wx0), fmul(x[y1][x1][c], wx1))
 *     v  = fadd(fmul(t0, wy0), fmul(t1, wy1))                            then vertical
 * (a weight of zero still multiplies: 0 * inf is a NaN here as it is in IEEE arithmetic).
 * Argmax: best = -inf, label = 0; classes in ascending order, class c is taken iff v > best (strict). So the lowest index wins a tie, a NaN
 * never wins, and a pixel whose every v is NaN or -inf has label 0 and score -inf. */
int mbn_upsample_argmax_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                            int factor, void *stream);
/* Dense head at the source resolution: the same read-out to ANY output size, out_rows x out_cols instead of rows*factor x cols*factor, in one
 * kernel that never writes the resampled tensor (mbn_f32_resample.hip). What a segmentation user does after a stretch resize:
 * resample the coarse logits to the photograph's own size, then take the argmax. logits: fp32 NHWC [batch][rows][cols][classes]; labels_i32 and
 * score_f32 (may be NULL): [batch][out_rows][out_cols].
 * The arithmetic, normative (tests/dense_any_ref.py reproduces it bit for bit in numpy). For an axis with n coarse samples and N output samples,
 * at output coordinate o, with half-pixel centres as torch.nn.functional.interpolate(mode="bilinear", align_corners=False):
 *     num = max((2*o + 1) * n - N, 0);   den = 2 * N;                                  (integers)
 *     i0  = num / den;   i1 = min(i0 + 1, n - 1);
 *     w1  = (float)((double)(num % den) / (double)den);   w0 = 1.0f - w1;
 * The quotient is formed in fp64 and rounded once to fp32 (numpy reproduces that bit for bit, and it does not depend on how a build compiles a
 * float division). The interpolation and the argmax are exactly those of mbn_upsample_argmax_f32 above: horizontal first (t0, t1 from x0, x1 and
 * wx0, wx1), then vertical (v from t0, t1 and wy0, wy1), fmul / fadd each rounded with no contraction, a zero weight still multiplies; classes in
 * ascending order, class c taken iff v > best (strict), label 0 and score -inf when nothing wins. For N = n * S, S = 8, 16 or 32, the rule
 * gives the weights and therefore the results of mbn_upsample_argmax_f32 bit for bit.
 * Envelope: out_rows >= 4 * rows and out_cols >= 4 * cols (a 32 x 32 output tile then touches at most 10 x 10 coarse vectors and a lane's four
 * rows at most three coarse rows), out_rows and out_cols at most 16384 ((2o + 1) * n stays inside int32), an image's logits and an image's output
 * map each below 2^31 bytes, batch <= 65535: otherwise MBN_EUNSUPPORTED and nothing is launched. NULL labels / logits, a non-positive size or a
 * pointer off 4 bytes: MBN_EINVAL. `logits` on 16 bytes with classes % 4 == 0 loads 16 bytes at a time; same results.
 * Ragged form: ONE launch reads out `batch` images of one coarse shape, each to its own size and place. An image is an mbn_label_item: its
 * output is rows x cols, at labels + dst_offset (and score + dst_offset), dst_offset in ELEMENTS. Items may come in any order; their maps must
 * not overlap.
 *   mbn_ragged_readout_create       allocates everything once: the items of max_batch (1..65535) images on the device and a pinned host copy.
 *                                   The handle belongs to the context: mbn_shutdown frees the ones still alive
 *   mbn_ragged_readout_set          checks every item against the coarse shape rows x cols x classes (MBN_EINVAL: a non-positive size, a negative
 *                                   offset, overlapping maps, batch outside 1..max_batch; MBN_EUNSUPPORTED: an item outside the per-image
 *                                   envelope above) and enqueues ONE asynchronous copy of the items on `stream`. No allocation. A REFUSED set
 *                                   changes nothing: the previous set stays valid. It first waits for the handle's previous copy and launches,
 *                                   whatever their streams. A set is not part of a graph (a capturing `stream`: MBN_EINVAL)
 *   mbn_resample_argmax_ragged_f32  the launch, asynchronous on `stream`, ordered behind the set by the stream. logits [batch][rows][cols][classes]
 *                                   of the set. No host allocation and no blocking call: it may be captured as one kernel node; a captured launch
 *                                   belongs to the set it was captured under and replayed after another set it does nothing. The mbn_alloc bounds
 *                                   rule applies: labels / score span max(dst_offset + rows * cols) elements. Nothing between the maps is written */
int mbn_resample_argmax_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                            int out_rows, int out_cols, void *stream);
typedef struct mbn_label_item { int64_t dst_offset; int32_t rows, cols; } mbn_label_item;   /* 16 bytes; dst_offset in ELEMENTS from labels (and score) */
typedef struct mbn_ragged_readout mbn_ragged_readout;
int mbn_ragged_readout_create(mbn_context *ctx, int max_batch, mbn_ragged_readout **r);
int mbn_ragged_readout_set(mbn_ragged_readout *r, int rows, int cols, int classes, const mbn_label_item *items, int batch, void *stream);
int mbn_resample_argmax_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *score_f32, const void *logits, void *stream);
int mbn_ragged_readout_destroy(mbn_ragged_readout *r);
/* Segment through the letterbox: the same read-out of a WINDOW of the network's input instead of the whole coarse map, so that the labels of an
 * image that went through MBN_FIT_PAD come out at the source size, one per source pixel, without the distortion of a stretch.
 * The coarse map has n samples along an axis and covers R network-input pixels (R = in_rows or in_cols; R / n need not be an integer). A window
 * [b, b + l) of those R pixels (integers, b >= 0, l >= 1, b + l <= R) is resampled to N outputs: output o sits at input coordinate
 * b + (o + 1/2) * l / N, that is at map coordinate u = (b + (o + 1/2) * l / N) * n / R - 1/2. Normative (tests/dense_window_ref.py reproduces it bit
 * for bit in numpy), all integers 64-bit:
 *     num = max((2*o + 1) * l * n + 2 * b * n * N - N * R, 0);   den = 2 * N * R;
 *     i0  = num / den;   i1 = min(i0 + 1, n - 1);
 *     w1  = (float)((double)(num % den) / (double)den);   w0 = 1.0f - w1;
 * i0 <= n - 1 follows from b + l <= R. There is NO clamp at the window's edge: an output next to the letterbox border interpolates with the coarse
 * samples outside the rectangle, which is the true bilinear value of the logits there (a zero weight still multiplies). The interpolation order, the
 * per-operation rounding and the argmax rule are those of mbn_resample_argmax_f32 unchanged. With b = 0, l = R the rule is mbn_resample_argmax_f32's
 * bit for bit (num and den are R times its own: the same rational, both fp64 operands exact); a window with R * N / l and b * N / l integers gives
 * rows b * N / l ... of mbn_resample_argmax_f32's resample to R * N / l bit for bit.
 * rect = (x, y, iw, ih), ordered as mbn_fit_pad writes it: columns [x, x + iw), rows [y, y + ih) of the in_rows x in_cols input.
 *   mbn_resample_argmax_window_f32  logits [batch][rows][cols][classes] -> labels_i32 (and score_f32, may be NULL) [batch][out_rows][out_cols], one
 *                                   rectangle for the whole batch. MBN_EINVAL: NULL labels / logits / rect, a pointer off 4 bytes, a non-positive
 *                                   size, x < 0, y < 0, iw < 1, ih < 1, a rectangle reaching past in_cols / in_rows, in_rows < rows or
 *                                   in_cols < cols. MBN_EUNSUPPORTED unless out_rows * in_rows >= 4 * ih * rows and out_cols * in_cols >=
 *                                   4 * iw * cols (the tile then touches at most 10 x 10 coarse vectors, as above), the output sides, in_rows and
 *                                   in_cols are at most 16384 (num < 2^46 and den <= 2^29 are then exact in fp64) and the byte and batch limits of
 *                                   mbn_resample_argmax_f32 hold. Nothing is launched on a refusal. The mbn_alloc bounds rule applies
 *   mbn_ragged_readout_set_window   a set whose image i has its own rectangle: mbn_label_window_item, 32 bytes (mbn_label_item keeps its 16). The
 *                                   checks of mbn_ragged_readout_set plus the ones above per item; a REFUSED set changes nothing. After it
 *                                   mbn_resample_argmax_ragged_f32 launches the window kernel, after a plain set the kernel it always launched. A
 *                                   captured launch replayed after ANY later set, of either kind, does nothing */
typedef struct mbn_label_window_item { int64_t dst_offset; int32_t rows, cols; int32_t x, y, iw, ih; } mbn_label_window_item;
int mbn_resample_argmax_window_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                                   int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols, void *stream);
int mbn_ragged_readout_set_window(mbn_ragged_readout *r, int rows, int cols, int classes, int in_rows, int in_cols,
                                  const mbn_label_window_item *items, int batch, void *stream);
/* Segment with confidence: the same read-outs, which also give the softmax probability of the winning class at every output pixel and can replace
 * the label of a pixel below a threshold. The full [out_rows][out_cols][classes] probabilities are never formed in memory.
 * Normative:
 *   Interpolants. For an output pixel the v_c, c = 0 .. classes - 1, are exactly the interpolated logits of mbn_resample_argmax_f32 (of
 *     mbn_resample_argmax_window_f32 for the window and a window set); best and label are exactly theirs. The labels (at min_prob = 0) and the
 *     score bits of these calls equal those of the argmax calls on the same arguments, bit for bit.
 *   Probability. prob = 1 / sum_c e(v_c), e(v) = exp(v - best) when v is not NaN, e(v) = 0 when v is NaN (a NaN never wins and adds nothing).
 *     If best is not finite, prob = 0: a pixel where nothing won (-inf) and a +inf winner; it falls under any positive threshold.
 *   Tolerance. prob is fp32 and NOT bit-pinned: exp and the order of the summation are the implementation's. Wherever the reference prob is
 *     nonzero the relative error is at most (classes + 200) * 2^-24; where it is 0 (a non-finite best) prob is exactly 0. The reference is the
 *     float64 evaluation of the formula on the fp32 v_c (tests/dense_prob_ref.py). Where the bound comes from: classes - 1 roundings of a
 *     sequential fp32 sum of non-negative terms; the rounding of v - best (or v - a reference near best) and of a log2(e) pre-multiply, each an
 *     absolute error of at most |d| * 2^-24 in the exponent of a term that weighs e^d (|d| e^d < 1 for d <= 0, |d| < 88 before underflow; for a
 *     reference at most 16 below best, d <= 16: at most 2.5 * 16 + 1 = 41 units for a term, once more for ONE rescale of the sum that counts and
 *     once more for exp(best - reference), 123 in all); exp within 2 ulp; the final division. The bound holds for EVERY input: the kernel does
 *     not rescale its sum at every new maximum (on an ascending ramp that would add one exp error per class) but only when a logit exceeds the
 *     sum's reference by more than 16, which leaves the rescaled part below classes * e^-16 of the sum from the second rescale on.
 *   Threshold. min_prob in [0, 1]; a NaN or a value outside is MBN_EINVAL. The stored label is ignore_label (any int32) iff the stored prob <
 *     min_prob: strict, on the fp32 value the kernel writes. min_prob = 0 never replaces a label. prob and score are written unchanged either way.
 * score_f32 may be NULL. prob_f32 may be NULL only when min_prob > 0 (thresholded labels alone); NULL with min_prob = 0 is MBN_EINVAL: that is
 * the argmax call. prob_f32 has the shape and the dst_offset rule of score_f32 and must be on 4 bytes. The envelope, pointer, alignment and
 * byte limits and their statuses are exactly those of the argmax call of the same form; nothing is launched on a refusal; the mbn_alloc bounds
 * rule applies to prob_f32 as to score_f32. mbn_resample_softmax_ragged_f32 works after either kind of set (mbn_ragged_readout_set: the plain
 * kernel, _set_window: the window kernel) and keeps the generation rule: a captured launch replayed after a later set does nothing. The handle
 * and its items are unchanged. Each of the three is ONE kernel and may be captured as one kernel node. */
int mbn_resample_softmax_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                             int classes, int out_rows, int out_cols, float min_prob, int ignore_label, void *stream);
int mbn_resample_softmax_window_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows,
                                    int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                                    float min_prob, int ignore_label, void *stream);
int mbn_resample_softmax_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, float min_prob,
                                    int ignore_label, void *stream);
/* Segment with test-time augmentation: ONE read-out of K views of the same images, their interpolated logits averaged per class and pixel in front
 * of the compare (multi-scale + flip evaluation). A VIEW is one presentation of the source image to the network: the whole image
 * resized, its aspect kept, into the rectangle (x, y, iw, ih) of the in_rows x in_cols network input, mirrored left-to-right when mirror = 1, the
 * pad colour elsewhere (mbn_fit_view and mbn_resizer_create_view below make one). One net of fixed input size serves every view; scales above 1
 * would crop and are refused for the reason mbn_net_segment_fit refuses MBN_FIT_CROP. The K tensors [out_rows][out_cols][classes] are never formed.
 * logits is VIEW-MAJOR: [n_views][batch][rows][cols][classes] fp32, what one mbn_net_forward_dense of the batch * n_views staged canvases gives;
 * labels_i32, prob_f32 and score_f32 are [batch][out_rows][out_cols]. Normative (tests/dense_ensemble_ref.py reproduces it bit for bit in numpy):
 *   Interpolants. For view k the v_c^(k) at output (oy, ox) are exactly those of mbn_resample_argmax_window_f32 for the rectangle of view k, the
 *     rows evaluated at oy, the columns at ox when mirror = 0 and at out_cols - 1 - ox when mirror = 1: the same index and weight rule, horizontal
 *     first, every product and sum rounded on its own.
 *   Sum. s_c = v_c^(0), then s_c = s_c + v_c^(k) for k = 1 .. K - 1 in view order, each addition one fp32 rounding.
 *   Mean. t_c = s_c * invK, invK = 1.0f / (float)K, one rounding.
 *   Label. The argmax of t_c over the classes in ascending order, strict compare: a NaN never wins; label 0 and score -inf when nothing wins. The
 *     score is the winning t.
 *   Probability. prob, min_prob and ignore_label follow "segment with confidence" above applied to t_c: prob = 1 / sum_c e(t_c) within
 *     (classes + 200) * 2^-24 relative of the float64 evaluation on the fp32 t_c, exactly 0 when best is not finite; the stored label is
 *     ignore_label iff the stored prob < min_prob.
 * prob_f32 = NULL with min_prob = 0 is the argmax form: no exponential is evaluated. score_f32 may be NULL. K = 1 gives
 * mbn_resample_argmax_window_f32's labels and score bit for bit (a mirror aside), and so do 2 or 4 copies of one view over the same logits: the sum
 * and the product by 1/2 or 1/4 are exact.
 * MBN_EINVAL: a NULL labels / logits / views, a pointer off 4 bytes, n_views outside 1..MBN_ENSEMBLE_MAX_VIEWS, a view whose rectangle
 * mbn_resample_argmax_window_f32 calls MBN_EINVAL, whose mirror is not 0 / 1 or whose reserved words are not 0, a non-positive size, min_prob outside
 * [0, 1] or NaN, or an undersized tracked buffer (mbn_alloc's bounds rule; the logits span n_views * batch maps). MBN_EUNSUPPORTED: any view outside
 * mbn_resample_argmax_window_f32's envelope taken with batch * n_views images. Nothing is launched on a refusal. ONE kernel, the views by value in
 * its arguments: it may be captured as one kernel node. */
#define MBN_ENSEMBLE_MAX_VIEWS 8
typedef struct mbn_view { int32_t x, y, iw, ih; int32_t mirror; int32_t reserved[3]; } mbn_view;   /* 32 bytes; mirror 0 / 1; reserved 0 */
int mbn_resample_ensemble_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                              int classes, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols, float min_prob,
                              int ignore_label, void *stream);
/* Segment by sliding window: ONE read-out of a grid of overlapping TILES of the same images, their interpolated logits averaged per class and pixel
 * where tiles overlap, in front of the compare. A tile is a tile_rows x tile_cols crop of the source image that the network saw
 * as one input of its own; the grid covers the image, so every source pixel has the logits of a crop at the crop's own scale instead of one
 * coarse vector of the whole image squeezed into the network's input. The tensors [out_rows][out_cols][classes] are never formed.
 * The plan. mbn_slide_axis places the tiles of one axis: regular steps, the last tile moved back flush with the far edge. Normative:
 *     n = (size > tile ? ceil((size - tile) / stride) : 0) + 1;      pos[i] = min(i * stride, size - tile)
 * MBN_EINVAL: a non-positive argument, a NULL pointer or stride > tile (gaps). MBN_EUNSUPPORTED: tile > size (that image belongs to the letterbox),
 * stride < ceil(tile / 2) (more than three tiles over a coordinate) or n > MBN_SLIDE_MAX_AXIS. Nothing is written on a refusal. The positions are
 * strictly ascending from 0 to size - tile without a gap, the tiles over a coordinate are a contiguous index range of at most three, and the tile
 * edges cut the axis into at most 2n - 1 cells of constant coverage. mbn_slide_plan runs both axes and fills an mbn_slide (unused y[] / x[] are 0);
 * it writes nothing on a refusal.
 * A hand-made mbn_slide is legal. For an output of out_rows x out_cols the read-out checks, for y against tile_rows / out_rows and for x against
 * tile_cols / out_cols: MBN_EINVAL unless ny (nx) is in 1..MBN_SLIDE_MAX_AXIS, the tile side is positive, y[0] = 0 and y[ny - 1] = out_rows -
 * tile_rows, the positions are strictly ascending, y[i + 1] <= y[i] + tile_rows (no gap) and the unused entries are 0; then MBN_EUNSUPPORTED unless
 * y[i + 3] >= y[i] + tile_rows (at most three tiles over a coordinate).
 * The read-out. logits is IMAGE-MAJOR: fp32 [batch][ny * nx][rows][cols][classes], tile t = iy * nx + ix, what one mbn_net_forward_dense of the
 * staged tiles gives; labels_i32, prob_f32 and score_f32 are [batch][out_rows][out_cols]. Normative (tests/dense_slide_ref.py reproduces it bit
 * for bit in numpy):
 *   Interpolants. Tile (iy, ix) covers output rows [y[iy], y[iy] + tile_rows) and columns [x[ix], x[ix] + tile_cols). At a pixel (oy, ox) it covers,
 *     its v_c are exactly the interpolants of mbn_resample_argmax_f32 for that tile's map resampled to tile_rows x tile_cols, at
 *     (oy - y[iy], ox - x[ix]): the same index and weight rule, horizontal first, every product and sum rounded on its own, a zero weight still
 *     multiplies. Each tile is an image of its own: the rule's clamps act at the tile's edge.
 *   Sum. Over the covering tiles in ascending iy, then ascending ix: s_c = v_c of the first, then s_c = s_c + v_c for each further tile, one fp32
 *     rounding each.
 *   Mean. t_c = s_c * inv, inv = 1.0f / (float)count, count the number of covering tiles (1, 2, 3, 4, 6 or 9). One rounding.
 *   Label, score, prob, min_prob, ignore_label. Those of mbn_resample_ensemble_f32 applied to t_c: the argmax in ascending class order with a strict
 *     compare, the score the winning t; prob = 1 / sum_c e(t_c) within (classes + 200) * 2^-24 relative of the float64 evaluation on the fp32 t_c,
 *     exactly 0 when best is not finite; the stored label is ignore_label iff the stored prob < min_prob.
 * prob_f32 = NULL with min_prob = 0 is the argmax form: no exponential is evaluated. score_f32 may be NULL. Where count = 1 the labels and score
 * bits are those of mbn_resample_argmax_f32 of that tile to tile_rows x tile_cols, so a plan of one tile is that call bit for bit; where count
 * is 2 or 4 the product by inv is exact.
 * MBN_EINVAL: NULL labels / logits / s, a pointer off 4 bytes, a non-positive size, a plan breaking the MBN_EINVAL rules above, min_prob outside
 * [0, 1] or NaN, or an undersized tracked buffer (mbn_alloc's bounds rule; the logits span batch * ny * nx maps). MBN_EUNSUPPORTED: more than three
 * tiles over a coordinate, tile_rows < 4 * rows or tile_cols < 4 * cols, a side above 16384, or the byte and batch limits of
 * mbn_resample_argmax_f32 (taken with batch * ny * nx maps). Nothing is launched on a refusal. ONE kernel, the plan by value in its arguments, no
 * device allocation and no blocking call: it may be captured as one kernel node. */
#define MBN_SLIDE_MAX_AXIS 16
typedef struct mbn_slide { int32_t tile_rows, tile_cols, ny, nx; int32_t y[MBN_SLIDE_MAX_AXIS], x[MBN_SLIDE_MAX_AXIS]; } mbn_slide;  /* 144 bytes; unused y[] / x[] are 0 */
int mbn_slide_axis(int size, int tile, int stride, int32_t *pos, int32_t *n);
int mbn_slide_plan(int in_rows, int in_cols, int tile_rows, int tile_cols, int stride_rows, int stride_cols, mbn_slide *s);
int mbn_resample_slide_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                           int classes, const mbn_slide *s, int out_rows, int out_cols, float min_prob, int ignore_label, void *stream);
/* Segment with runners-up: the read-out at any output size that gives the k best classes of every output pixel with their scores and softmax
 * probabilities instead of the winner alone: the margin between first and second place, relabelling from a short list, "is the
 * truth among the five best" (rank score, below). The dense counterpart of mbn_softmax_topk_f32. The tensor [out_rows][out_cols][classes] is never
 * formed. Layout, RANK-MAJOR: labels_i32, prob_f32 and score_f32 are [k][batch][out_rows][out_cols]; plane 0 is, in shape and place, the
 * [batch][out_rows][out_cols] map every later stage takes (mbn_confusion_i32, mbn_components_i32, the boundary and panoptic calls).
 * Ragged form: rank j of item i is at j * plane_stride + dst_offset_i, plane_stride in ELEMENTS and at least the set's span
 * max(dst_offset + rows * cols); nothing between the maps is written, in any plane.
 * Normative (tests/dense_topk_ref.py reproduces it in numpy):
 *   Interpolants. The v_c, c = 0 .. classes - 1, of an output pixel are exactly those of mbn_resample_argmax_window_f32 for `rect` (for a window
 *     set: of its item's rectangle); for a NULL rect or a plain set those of mbn_resample_argmax_f32. The same index and weight rule, horizontal
 *     first, every product and sum rounded on its own. (The kernel evaluates the window rule throughout: a NULL rect is the window (0, 0, cols,
 *     rows) of a rows x cols input, which is mbn_resample_argmax_f32's rule bit for bit, see "segment through the letterbox".)
 *   Selection. State: slots j = 0 .. k - 1, each (val_j, lab_j), every val = -inf. The classes are visited in ascending order. Class c enters iff
 *     v_c > val_{k-1} (strict: a NaN never enters, -inf never enters). It goes to the smallest j with v_c > val_j, and slots j .. k - 2 move down
 *     one. So the slots are sorted by value, descending, and equal values keep ascending class order. Slot 0 is exactly the argmax read-out's
 *     (best, label), and the first k' slots of a call with k are the slots of a call with k' (PREFIX property).
 *   Unfilled slots. A slot whose val is still -inf at the end stores score -inf and prob 0; its label is 0 at rank 0 (the argmax rule: plane 0
 *     stays bit-equal to the argmax read-out) and -1 at ranks >= 1.
 *   Probability. prob_j = e(val_j) / sum_c e(v_c), with e and the sum exactly as in "segment with confidence" (e(v) = exp(v - best), 0 for a NaN):
 *     the same lazy-reference operations in the same order, so prob_0 has the bits mbn_resample_softmax_f32 writes. prob_j = 0 exactly when best
 *     is not finite or slot j is unfilled. Elsewhere, against the float64 evaluation on the fp32 v_c,
 *         |prob_j - ref_j| <= (classes + 200 + 2 * |val_j - best|) * 2^-24 * ref_j + 2^-125.
 *     Derivation. The denominator and the division are those of prob_0: (classes + 200) * 2^-24 covers them, with the 123 units "segment with
 *     confidence" spends on exponents whose argument is at most 16 in magnitude: 41 of them for the numerator exp(best - reference). Here the
 *     numerator is exp2((val_j - reference) * log2(e)) with d = val_j - reference, |d| <= |val_j - best| + 16. The subtraction and the pre-multiply
 *     each round once, an absolute error of at most |d| * 2^-24 (natural units; the factor log2(e) cancels against the ln 2 of exp2's derivative)
 *     in the exponent each, which is a RELATIVE error of the numerator: 2 * |val_j - best| units on top of 2 * 16 = 32 of the 41 already counted
 *     (the rest is exp's 2 ulp and slack). A numerator below 2^-126 may be flushed to 0 by the exponential; over a sum >= 1 that is an absolute
 *     error below 2^-126, and one more halving of slack gives the 2^-125.
 *   Threshold. min_prob and ignore_label act on PLANE 0 ONLY, exactly as in mbn_resample_softmax_f32: the stored label of rank 0 is ignore_label
 *     iff the stored prob_0 < min_prob (strict). The planes >= 1, every prob and every score are written unchanged.
 *   Logit form. prob_f32 = NULL with min_prob = 0: no exponential is evaluated (the ensemble's convention). score_f32 may be NULL.
 * MBN_EINVAL: k outside 1..MBN_TOPK_MAX, k > classes, whatever the softmax call of the same form calls MBN_EINVAL (a NULL rect is no error here: it
 * is the whole map), plane_stride below the set's span, a handle without a set, or an undersized tracked buffer (mbn_alloc's bounds rule: each
 * output spans (k - 1) * plane + span elements, plane = batch * out_rows * out_cols or plane_stride). MBN_EUNSUPPORTED: outside the window (rect
 * given) or argmax (NULL) envelope; and k * plane above 2^40 elements: the kernel reaches rank j of image i through a 64-bit element base
 * j * plane + i * out_rows * out_cols and 32-bit offsets inside a map, so only that base limits the planes, and 2^40 keeps every byte count exact.
 * Nothing is launched on a refusal. ONE kernel per call, which may be captured as one kernel node; the ragged form works after either kind of set
 * and keeps the generation rule (a captured launch replayed after a later set writes nothing). mbn_resample_topk_envelope answers the shape part
 * of the uniform form; pure host. */
#define MBN_TOPK_MAX 8
int mbn_resample_topk_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                          int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols, int k, float min_prob,
                          int ignore_label, void *stream);
int mbn_resample_topk_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int k,
                                 int64_t plane_stride, float min_prob, int ignore_label, void *stream);
int mbn_resample_topk_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows,
                               int out_cols, int k);
/* Score a segmentation: the confusion matrix of the label maps the read-outs above write against a ground truth, accumulated on the device, and
 * the standard metrics of such a matrix on the host. The dense counterpart of mbn_softmax_topk_f32.
 * Normative (tests/confusion_ref.py reproduces it in numpy; the arithmetic is integer, so every result is exact and does not depend on the order
 * in which the device's atomics arrive):
 *   counts is uint64_t [classes + 1][classes + 1], row-major, on 8 bytes. The ROW is the truth; row `classes` is VOID: a truth value outside
 *     [0, classes), for example the usual 255. The COLUMN is the prediction; column `classes` is ABSTAINED: a label outside [0, classes): the
 *     ignore_label the thresholded read-outs store, and any other int32, negative values included.
 *   Every pixel adds exactly 1 to exactly one cell. The call ADDS to counts: the caller clears it (mbn_memset) and a dataset accumulates over many
 *     calls. After any sequence of calls the sum of all cells equals the number of pixels scored.
 *   Truth is uint8 (truth_bytes = 1) or int32 (truth_bytes = 4). A uint8 value v goes to row v < classes ? v : classes; an int32 value likewise,
 *     negative values to the void row.
 *   mbn_confusion_i32         `count` pixels: labels_i32 [count], truth [count]. labels_i32 may be any pointer on 4 bytes, a uint8 truth any byte
 *                             pointer, an int32 truth any pointer on 4 bytes, independently of each other. ONE kernel, asynchronous on `stream`
 *                             (NULL: the context's); it may be captured as one kernel node. The grid is persistent, sized from the planning CU
 *                             count (mbn_set_planning_cus); the counts are the same at every planning count
 *   mbn_confusion_ragged_i32  the maps of a ragged set: the pixels of item i are labels_i32 [dst_offset_i .. + rows_i * cols_i) and truth uses the
 *                             SAME element offsets; nothing between the maps is read. After either kind of set (the 16-byte and the 32-byte items
 *                             share their first 16 bytes). ONE kernel; it keeps the handle's generation rule (a captured launch replayed after a
 *                             later set does nothing) and the next set waits for it. `classes` is the call's and need not be the set's
 * MBN_EINVAL: a NULL pointer, counts_u64 off 8 bytes, labels_i32 off 4, an int32 truth off 4, classes < 1, count < 1, truth_bytes not 1 or 4, a
 * handle without a set, or an undersized tracked buffer (mbn_alloc's bounds rule: counts_u64 spans (classes + 1)^2 * 8 bytes; labels_i32 and
 * truth span `count` elements, in the ragged form max(dst_offset + rows * cols)). MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES or
 * count > 2^34. Nothing is launched on a refusal. mbn_confusion_envelope answers the shape part; mbn_confusion_form says which form of the kernel
 * a class count takes (0: a workgroup counts in LDS; 1: global atomics only; monotone, one switch point). Both are pure host functions.
 *   mbn_confusion_metrics     pure C in doubles, exact for counts below 2^53. n = counts, C = classes:
 *     valid = the sum of rows t < C over all columns; void_pixels = the sum of row C; abstained = sum over t < C of n[t][C]; pixels = valid + void.
 *     For class c: tp = n[c][c]; fn = (sum of row c) - tp (the abstained column counts as a miss); fp = sum over t < C, t != c of n[t][c] (the
 *     void row is excluded). iou_c = tp / (tp + fp + fn); a class is PRESENT iff that denominator is > 0, otherwise iou_c = NaN.
 *     pixel_accuracy = sum of tp / valid (0 when valid = 0); miou = the mean of iou_c over the present classes (0 when there are none);
 *     mean_accuracy = the mean of tp / (tp + fn) over the classes with tp + fn > 0 (0 when there are none);
 *     fw_iou = sum over the present classes of ((tp + fn) / valid) * iou_c; classes_present = the number of present classes.
 *     Every ratio is one division of exact integers; the means are summed in ascending class order. iou: [classes] or NULL.
 *     MBN_EINVAL: NULL counts or m, classes < 1; MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES. */
#define MBN_CONFUSION_MAX_CLASSES 4096
typedef struct mbn_seg_metrics {
    double pixels, valid, void_pixels, abstained;
    double pixel_accuracy, mean_accuracy, miou, fw_iou;
    int32_t classes_present, reserved;
} mbn_seg_metrics;
int mbn_confusion_i32(mbn_context *ctx, void *counts_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes, int64_t count,
                      void *stream);
int mbn_confusion_ragged_i32(mbn_ragged_readout *r, void *counts_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes,
                             void *stream);
int mbn_confusion_envelope(int classes, int truth_bytes, int64_t count);
int mbn_confusion_form(int classes);
int mbn_confusion_metrics(const uint64_t *counts, int classes, mbn_seg_metrics *m, double *iou);
/* Rank score: is the truth among the k best. The k rank-major label planes of mbn_resample_topk_f32 against a ground truth, accumulated on the
 * device: the dense counterpart of top-5 accuracy. Normative (tests/dense_topk_ref.py has the numpy form; the arithmetic is integer,
 * so the bytes are the same at every planning CU count, in both forms of the kernel and on graph replay):
 *   ranks is uint64_t [classes + 1][k + 1], row-major, on 8 bytes; the calls ADD to it. The ROW is the truth by mbn_confusion_i32's rule: uint8
 *     (truth_bytes = 1) or int32 (4), a value outside [0, classes) goes to row `classes`, VOID. Column j < k counts the pixels whose truth equals
 *     the rank-j label, for the smallest such j; column k counts the rest, every void pixel included. A label outside [0, classes) (ignore_label,
 *     the -1 of an unfilled slot) matches nothing. Every pixel adds 1 to exactly one cell: after any sequence of calls the cells sum to the pixels
 *     scored, and column 0 of row t is the diagonal cell [t][t] of mbn_confusion_i32 on plane 0.
 *   mbn_topk_rank_i32         `count` pixels: plane j is labels_i32 [j * plane_stride .. + count), plane_stride in ELEMENTS and at least count;
 *                             truth [count]. labels_i32 any pointer on 4 bytes, a uint8 truth any byte pointer, an int32 truth any pointer on 4
 *                             bytes. ONE kernel, asynchronous on `stream` (NULL: the context's), capturable as one kernel node; a persistent grid
 *                             sized from the planning CU count
 *   mbn_topk_rank_ragged_i32  the maps of a ragged set: item i's pixels are at dst_offset_i in every plane and in truth; plane_stride at least the
 *                             set's span. After either kind of set; ONE kernel; it keeps the generation rule and the next set waits for it
 * MBN_EINVAL: a NULL pointer, ranks_u64 off 8 bytes, labels_i32 off 4, an int32 truth off 4, k outside 1..MBN_TOPK_MAX, classes < 1, count < 1,
 * truth_bytes not 1 or 4, plane_stride below count (the span), a handle without a set, or an undersized tracked buffer (ranks_u64 spans
 * (classes + 1) * (k + 1) * 8 bytes, labels_i32 (k - 1) * plane_stride + count elements, truth count elements). MBN_EUNSUPPORTED: classes >
 * MBN_CONFUSION_MAX_CLASSES, count > 2^34 or k * plane_stride > 2^40. Nothing is launched on a refusal.
 *   mbn_topk_metrics          pure C in doubles, exact for counts below 2^53. n = ranks, C = classes: valid = the sum of the rows t < C;
 *     accuracy[j] = sum over t < C and i <= j of n[t][i], over valid (0 when valid = 0): top-(j + 1) pixel accuracy; mean_accuracy[j] = the mean over
 *     the classes with a non-empty row of (sum over i <= j of n[t][i]) / (the row's sum), in ascending class order (0 when there are none).
 *     accuracy and mean_accuracy are [k] or NULL, valid may be NULL. MBN_EINVAL: NULL ranks, classes < 1, k outside 1..MBN_TOPK_MAX;
 *     MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES. */
int mbn_topk_rank_i32(mbn_context *ctx, void *ranks_u64, const void *labels_i32, int k, int64_t plane_stride, const void *truth, int truth_bytes,
                      int classes, int64_t count, void *stream);
int mbn_topk_rank_ragged_i32(mbn_ragged_readout *r, void *ranks_u64, const void *labels_i32, int k, int64_t plane_stride, const void *truth,
                             int truth_bytes, int classes, void *stream);
int mbn_topk_metrics(const uint64_t *ranks, int classes, int k, double *accuracy, double *mean_accuracy, double *valid);
/* Calibration score: is the probability worth anything, and which min_prob to pass. The label maps and the softmax probabilities the read-outs
 * above write (mbn_resample_softmax_f32, its window and ragged forms, the ensemble, slide and top-k read-outs: plane 0 of a rank-major top-k call
 * is a valid input as it is) against a ground truth, accumulated on the device into one small table: the reliability diagram and expected
 * calibration error of Guo et al. 2017 and the risk-coverage curve of the min_prob threshold come from it on the host.
 * Normative (tests/calibration_ref.py is the numpy form):
 *   calib is uint64_t [bins + 1][4], row-major, on 8 bytes; the calls ADD to it. bins is in 1 .. MBN_CALIBRATION_MAX_BINS. For a pixel with label
 *   l (int32), probability x (fp32) and truth t (uint8 or int32 by mbn_confusion_i32's rule):
 *     p    x clamped: 0 when x is a NaN or x < 0, 1 when x > 1, else x. (The read-outs only write values in [0, 1]; the clamp defines the call for
 *          any buffer.)
 *     bin  min(bins - 1, (int32) trunc(p (*) (float) bins)): (*) is ONE fp32 multiplication, rounded to nearest, contracted with nothing.
 *          numpy: (p * np.float32(bins)).astype(np.int64). p = 1 goes to bin bins - 1.
 *     q    (uint64) trunc(p * 2^24): the product is exact in fp32 and q <= 2^24.
 *     t outside [0, classes): VOID. Adds 1 to [bins][0] and nothing else; the other three cells of row `bins` stay 0. Neither l nor x is read.
 *     else l outside [0, classes) (ignore_label, -1, any negative): ABSTAINED. Adds 1 to [bin][3].
 *     else ANSWERED: adds 1 to [bin][0], (l == t) to [bin][1] and q to [bin][2].
 *   Every pixel adds 1 to exactly one cell of columns 0 and 3: after any sequence of calls those two columns sum to the pixels scored. On the same
 *   labels and truth, against mbn_confusion_i32: the sum of [b][1] is the trace of its matrix over the valid rows, the sum of [b][3] its abstained
 *   column over the valid rows, [bins][0] the sum of its void row. Everything is integer once bin and q are formed per pixel, so the bytes do not
 *   depend on the order of the atomics: the same at every planning CU count and on graph replay. The fixed-point column [b][2] cannot wrap
 *   below 2^40 answered pixels in total (2^40 * 2^24 = 2^64); columns 0, 1 and 3 count pixels.
 *   mbn_calibration_f32         `count` pixels: labels_i32 [count], prob_f32 [count], truth [count]. labels_i32 and prob_f32 any pointers on 4
 *                               bytes, a uint8 truth any byte pointer, an int32 truth any pointer on 4 bytes, independently of each other. ONE
 *                               kernel, asynchronous on `stream` (NULL: the context's), capturable as one kernel node; a persistent grid sized
 *                               from the planning CU count
 *   mbn_calibration_ragged_f32  the maps of a ragged set: item i's pixels are at dst_offset_i in labels_i32, in prob_f32 and in truth; nothing
 *                               between the maps is read. After either kind of set; ONE kernel; it keeps the generation rule (a captured launch
 *                               replayed after a later set adds nothing) and the next set waits for it
 * MBN_EINVAL: a NULL pointer, calib_u64 off 8 bytes, labels_i32 or prob_f32 off 4, an int32 truth off 4, classes < 1, count < 1, truth_bytes not 1
 * or 4, bins < 1, a handle without a set, or an undersized tracked buffer (calib_u64 spans (bins + 1) * 32 bytes; labels_i32, prob_f32 and truth
 * span `count` elements, in the ragged form the set's span). MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES, bins >
 * MBN_CALIBRATION_MAX_BINS or count > 2^34. Nothing is launched on a refusal. mbn_calibration_envelope answers the shape part; pure host.
 *   mbn_calibration_metrics     pure C in doubles, exact for cells below 2^53. accuracy, confidence, coverage and selective_accuracy are [bins] or
 *     NULL. For bin b: n_b = [b][0]; accuracy[b] = [b][1] / n_b; confidence[b] = [b][2] / (n_b * 2^24); both NaN when n_b = 0. With N = the sum
 *     of n_b: pixels = N + abstained + void_pixels; answered = N; abstained = the sum of [b][3]; void_pixels = [bins][0]; accuracy = (the sum of
 *     [b][1]) / N and mean_confidence = (the sum of [b][2]) / (N * 2^24), both 0 when N = 0; ece = the sum over the non-empty bins, in ascending
 *     order, of (n_b / N) * |accuracy[b] - confidence[b]|; mce = the largest such gap (both 0 when N = 0).
 *     The curve, for edge j = 0 .. bins - 1, is that of keeping the bins >= j: coverage[j] = (the sum over b >= j of [b][0]) / (N + abstained)
 *     (0 when that is 0: the pixels already abstained count against the coverage and are not brought back by a lower edge);
 *     selective_accuracy[j] = (the sum over b >= j of [b][1]) / (the sum over b >= j of [b][0]), NaN when that is empty;
 *     aurc = the sum over j of (1 - selective_accuracy[j]) * (coverage[j] - coverage[j + 1]) with coverage[bins] = 0, empty terms skipped.
 *     Every ratio is one division of exact integers. MBN_EINVAL: NULL calib or m, bins < 1; MBN_EUNSUPPORTED: bins > MBN_CALIBRATION_MAX_BINS.
 *   mbn_calibration_threshold   the smallest edge j whose selective_accuracy[j] >= target_accuracy: *min_prob = (float) j / (float) bins with that
 *     edge's coverage and selective accuracy (each output may be NULL). MBN_EINVAL: as above, or a target outside [0, 1] (a NaN included).
 *     MBN_ENOTFOUND when no edge reaches the target (every edge is empty, or the best kept set is still below it): nothing is written.
 *   The power-of-two guarantee. For bins a power of two, p (*) bins is exact and (float) j / bins is exact, so bin >= j holds exactly when
 *     p >= j / bins: the complement of the read-outs' strict test prob < min_prob at min_prob = j / bins. Edge j of the curve is then exactly what
 *     a read-out with that min_prob will keep (tests/test_calibration_cpu.py proves it on every edge and its neighbours). For other bin counts the
 *     curve is that of the bins, with no such guarantee. */
#define MBN_CALIBRATION_MAX_BINS 1024
typedef struct mbn_calibration {
    double pixels, answered, abstained, void_pixels;
    double accuracy, mean_confidence, ece, mce, aurc;
} mbn_calibration;
int mbn_calibration_f32(mbn_context *ctx, void *calib_u64, const void *labels_i32, const void *prob_f32, const void *truth, int truth_bytes,
                        int classes, int bins, int64_t count, void *stream);
int mbn_calibration_ragged_f32(mbn_ragged_readout *r, void *calib_u64, const void *labels_i32, const void *prob_f32, const void *truth,
                               int truth_bytes, int classes, int bins, void *stream);
int mbn_calibration_envelope(int classes, int truth_bytes, int bins, int64_t count);
int mbn_calibration_metrics(const uint64_t *calib, int bins, mbn_calibration *m, double *accuracy, double *confidence, double *coverage,
                            double *selective_accuracy);
int mbn_calibration_threshold(const uint64_t *calib, int bins, double target_accuracy, float *min_prob, double *coverage,
                              double *selective_accuracy);
/* Score the probabilities: negative log-likelihood and Brier score of the WHOLE softmax distribution of every output pixel against a ground truth,
 * at up to eight temperatures in one pass. ECE (above) says whether the winner's confidence is honest; these two proper scoring
 * rules say whether the distribution is, and the NLL is what a temperature is fitted on (Guo et al. 2017). The read-out takes the truth INTO the
 * class loop: the tensor [out_rows][out_cols][classes] is never formed. Normative (tests/dense_nll_ref.py is the float64 form):
 *   Interpolants. For an output pixel, v_c, best and label are exactly the interpolants, maximum and argmax of mbn_resample_argmax_f32; with a
 *     rect (a window set) those of mbn_resample_argmax_window_f32. (The kernel evaluates the window rule throughout, as the top-k read-out does: a
 *     NULL rect is the window (0, 0, cols, rows) of a rows x cols input, bit for bit the plain rule.)
 *   Truth. t is the pixel's truth at the OUTPUT resolution, [batch][out_rows][out_cols] (ragged: at the items' dst_offsets), uint8 (truth_bytes
 *     = 1) or int32 (4). A value outside [0, classes) is VOID, as in mbn_confusion_i32.
 *   Temperatures. inv_temps[j], j < temps, is a HOST array of fp32 inverse temperatures beta_j = 1 / T_j; 1 <= temps <= MBN_NLL_MAX_TEMPS; each
 *     beta_j is finite and in [1/16, 16]. It is read at the call and travels in the kernel's arguments.
 *   Scores. Per temperature, in real arithmetic on the fp32 v_c and the fp32 beta:
 *       x_c = beta (v_c - best);  e_c = exp(x_c), 0 for a NaN v_c;  S = sum_c e_c;  Q = sum_c e_c^2;
 *       nll = log S - x_t;        brier = 1 - 2 e_t / S + Q / S^2        (= sum_c (p_c - [c == t])^2 with p_c = e_c / S).
 *     best not finite (the prob = 0 case of "segment with confidence"): nll = MBN_NLL_CAP, brier = 1. v_t a NaN or -inf under a finite best:
 *     nll = MBN_NLL_CAP, brier = 1 + Q / S^2. The stored nll is clamped to [0, MBN_NLL_CAP], the stored brier to [0, 2]. The NLL is formed in the
 *     log domain: it stays finite where p_t underflows (a ramp of 65 logit units at beta = 16 gives about 1040, not the cap).
 *   Outputs. nll_f32 and brier_f32 are optional, independent of each other, on 4 bytes; each holds `temps` planes, temperature-major:
 *     [temps][batch][out_rows][out_cols]; ragged: plane j of item i at j * plane_stride + dst_offset_i ELEMENTS, plane_stride at least the set's
 *     span (the rule of the top-k planes), nothing between the maps written. A void pixel stores -1.0f in both; no scored pixel can.
 *     nll_u64 is required: uint64 [temps][classes + 1][4] on 8 bytes, ADDED to (the caller clears it, mbn_memset). A scored pixel adds to row t
 *     of EVERY plane j: 1 to column 0, trunc(nll * 2^16) to column 1, trunc(brier * 2^24) to column 2 and (label == t) to column 3, nll and
 *     brier being the fp32 values the kernel stores (or would store) for plane j: both products are exact in fp32. A void pixel adds 1 to
 *     [j][classes][0] and nothing else. Column 1 cannot wrap below 2^33 pixels (2^31 a pixel at the cap), column 2 below 2^39.
 *   Determinism. A pixel's values do not depend on the launch and everything after the quantisation is integer: the table and the maps are the
 *     same bytes at every planning CU count and on graph replay.
 *   Independence. The arithmetic of temperature j does not depend on temps, on the other entries or on the instantiation that serves the call:
 *     plane j of a call with 8 temperatures equals the single plane of a call with beta_j alone, bit for bit.
 *   Tolerance. The maps are fp32 and NOT bit-pinned against the reference (the float64 evaluation of the formulas on the fp32 v_c). Outside the
 *     capped cases, as ABSOLUTE errors:  |nll - ref| <= (classes + 200 + 4 |x_t|) * 2^-24,   |brier - ref| <= 4 (classes + 200) * 2^-24.
 *     Derivation for the implementation (csrc/mbn_f32_resample.hip, NLL): two passes, the second with the FINAL best, so every d = v_c - best is
 *     <= 0 and nothing overflows at beta = 16. e_c = exp2(d * k), k = fp32(beta * log2 e) formed on the host: the subtraction, the rounding of k
 *     and the product each put at most |x_c| * 2^-24 (natural units) into the exponent of a term that weighs e^x (|x| e^x < 1 for x <= 0), 3
 *     units a term at most; exp2 within 2 ulp; a sequential fp32 sum of non-negative terms, classes - 1 roundings: S is relative-exact within
 *     (classes + 5) * 2^-24, far inside the classes + 200 of "segment with confidence". Q's terms carry twice the exponent error plus one
 *     rounding of the square: within (classes + 9) * 2^-24. log turns the relative error of S into an absolute one, plus log2's 1 ulp and the
 *     product by ln 2 on a value of at most ln classes < 9: under classes + 25 units. x_t = beta * (v_t - best) is one subtraction and one
 *     product: 1.5 |x_t| units; the last subtraction rounds at the size of nll <= |x_t| + ln classes: another |x_t| / 2 + 5 units. In all under
 *     (classes + 30 + 2 |x_t|) * 2^-24: the bound above with room. Brier is three terms of magnitude at most 2: 2 e_t / S (the error of e_t, of
 *     S and of 1 / S, times 2), Q / S^2 (Q's error and S's twice) and two additions: under 4 (classes + 20) * 2^-24. A term below 2^-126 may be
 *     flushed to 0 by the exponential: an absolute 2^-126 a class against S >= 1.
 *   mbn_resample_nll_f32         logits [batch][rows][cols][classes]; rect = NULL is the whole map, as in mbn_resample_topk_f32 (in_rows and
 *                                in_cols are then not read). ONE kernel, asynchronous on `stream` (NULL: the context's), capturable as one node
 *   mbn_resample_nll_ragged_f32  the maps of a ragged set, after either kind of set. ONE kernel; it keeps the generation rule: a captured
 *                                launch replayed after a later set adds nothing and writes nothing; the next set waits for it
 * MBN_EINVAL: NULL ctx / nll_u64 / logits / truth / inv_temps, nll_u64 off 8 bytes, a map or the logits off 4, an int32 truth off 4 (a uint8
 * truth may be any byte pointer), truth_bytes not 1 or 4, temps outside 1..MBN_NLL_MAX_TEMPS, a beta that is NaN, infinite or outside [1/16, 16],
 * whatever the argmax (NULL rect) or window call of the same shape calls MBN_EINVAL, plane_stride below the set's span, a handle without a set, or
 * an undersized tracked buffer (mbn_alloc's bounds rule: the table spans temps * (classes + 1) * 32 bytes, a map (temps - 1) * plane + span
 * elements, truth span elements). MBN_EUNSUPPORTED: outside the envelope of that argmax or window call, classes > MBN_CONFUSION_MAX_CLASSES, or
 * temps * plane above 2^40 elements (mbn_resample_topk_ragged_check's limit). An MBN_EINVAL goes in front of an MBN_EUNSUPPORTED. Nothing is
 * launched or written on a refusal. mbn_resample_nll_envelope answers the shape part of the uniform call; pure host.
 *   mbn_nll_metrics  pure C in doubles, exact for cells below 2^53; plane j of the table. scored = the sum of column 0 over the class rows;
 *     void_pixels = [j][classes][0]; pixels = scored + void_pixels; nll = (sum of column 1) / (scored * 2^16); brier = (sum of column 2) /
 *     (scored * 2^24); accuracy = (sum of column 3) / scored; all three 0 when nothing is scored. class_nll and class_brier are [classes] or NULL:
 *     the same ratios of one row, NaN for a class with an empty row; classes_present counts the others and mean_class_nll / mean_class_brier
 *     are the means over them in ascending class order (0 when there are none). Every ratio is one division of exact integers.
 *     MBN_EINVAL: NULL table or m, classes < 1, temps outside 1..MBN_NLL_MAX_TEMPS, j outside [0, temps); MBN_EUNSUPPORTED: classes >
 *     MBN_CONFUSION_MAX_CLASSES.
 *   mbn_nll_best     which plane of a temperature grid has the smallest NLL. inv_temps must be strictly ascending (and positive, finite), else
 *     MBN_EINVAL. *best = the plane with the smallest INTEGER sum of column 1 over the class rows, the lowest index on a tie; MBN_ENOTFOUND
 *     (nothing written) when plane 0 scored nothing. *at_edge = 1 when temps > 1 and best is the first or last plane: the caller should widen
 *     the grid. *inv_temp = beta_best, refined when best is interior and the parabola through the three points (x_i, y_i) = (ln beta_i, sum_i),
 *     i = best - 1, best, best + 1, opens upward: with s01 = (y1 - y0) / (x1 - x0), s12 = (y2 - y1) / (x2 - x1) and a = (s12 - s01) /
 *     (x2 - x0) > 0 the vertex is x* = (x0 + x1) / 2 - s01 / (2 a) (unequal spacing allowed), clamped to [x0, x2], and *inv_temp = exp(x*).
 *     inv_temp and at_edge may be NULL. The other statuses are mbn_nll_metrics'. */
#define MBN_NLL_MAX_TEMPS 8
#define MBN_NLL_CAP 32768.0f
typedef struct mbn_nll {
    double pixels, scored, void_pixels, nll, brier, accuracy, mean_class_nll, mean_class_brier;
    int classes_present;
} mbn_nll;
int mbn_resample_nll_f32(mbn_context *ctx, void *nll_u64, void *nll_f32, void *brier_f32, const void *logits, const void *truth, int truth_bytes,
                         int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                         const float *inv_temps, int temps, void *stream);
int mbn_resample_nll_ragged_f32(mbn_ragged_readout *r, void *nll_u64, void *nll_f32, void *brier_f32, int64_t plane_stride, const void *logits,
                                const void *truth, int truth_bytes, const float *inv_temps, int temps, void *stream);
int mbn_resample_nll_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                              int truth_bytes, int temps);
int mbn_nll_metrics(const uint64_t *nll_u64, int classes, int temps, int j, mbn_nll *m, double *class_nll, double *class_brier);
int mbn_nll_best(const uint64_t *nll_u64, int classes, int temps, const float *inv_temps, int *best, double *inv_temp, int *at_edge);
/* Regions of a label map: connected-component labelling of the int32 maps the read-outs above write, on the device.
 * Normative (tests/components_ref.py is the numpy form; everything is integer, so the result is a function of the input alone: the same bytes at
 * every planning CU count, in both forms, on every run and on graph replay). For one image L [rows][cols] and classes >= 1:
 *   A pixel whose label lies outside [0, classes) is ABSTAINED (the ignore_label of the thresholded read-outs, negatives, INT32_MAX): it belongs
 *     to no region and neither connects nor separates anything else.
 *   Two valid pixels are adjacent if they have the same label and are neighbours under `connectivity`: 4 = the edge neighbours, 8 = the edge and
 *     corner neighbours. A REGION is a connected component of that relation.
 *   A region's FIRST PIXEL is its smallest linear index r * cols + c. Regions are numbered 0 .. n - 1 per image in ascending order of their first pixel.
 *   min_area >= 1: a region of fewer than min_area pixels is DROPPED. Connectivity is decided before the drop; dropping does not merge the
 *     neighbours of a dropped region afterwards; the survivors are numbered as above among themselves. min_area = 1 keeps everything.
 * Outputs per image:
 *   comp_i32 [rows][cols]        the pixel's region number; -1 for abstained pixels and for pixels of dropped regions. May be NULL.
 *   n_regions_i32                the number of surviving regions: the true count, even above max_regions. Required.
 *   regions [max_regions]        mbn_region (32 bytes): record i describes region i; records >= min(n, max_regions) are NOT written. NULL iff
 *                                max_regions = 0.
 *   labels_out_i32 [rows][cols]  L with the pixels of dropped regions replaced by ignore_label; every other pixel copied, abstained ones included.
 *                                May be NULL. It (and comp_i32) must not overlap labels_i32.
 *   mbn_components_i32         maps [batch][rows][cols], the table [batch][max_regions], n_regions_i32 [batch]
 *   mbn_components_ragged_i32  the maps of a ragged set, of either item kind (only the items' first 16 bytes are used): comp_i32 and labels_out_i32
 *                              use the labels' dst_offset, nothing between the maps is read or written; the table is [set batch][max_regions].
 *                              It keeps the handle's generation rule (a captured launch replayed after a later set does nothing) and the next
 *                              set waits for it
 * Both are a FIXED sequence of seven kernels on `stream` (NULL: the context's) with no host decision between them, no host allocation, no copy to
 * the host and no blocking call: a call may be captured as a linear chain of kernel nodes. The grids are sized from the planning CU count. Calls on
 * one handle share its scratch: they must be ordered on one stream (or by the caller's events).
 * labels_i32, comp_i32, labels_out_i32, regions and n_regions_i32 may be any pointers on 4 bytes.
 * The handle holds all scratch (mbn_components_scratch_bytes (max_batch, max_pixels): 8 bytes per pixel + 4 bytes per 1024 pixels and per image),
 * allocated once by mbn_components_create; mbn_shutdown frees the handles still alive.
 * MBN_EINVAL: a NULL handle, labels_i32 or n_regions_i32; regions NULL with max_regions > 0; a pointer off 4 bytes; batch, rows, cols or
 * classes < 1; connectivity other than 4 or 8; min_area < 1; max_regions < 0; labels_out_i32 or comp_i32 overlapping labels_i32; batch above the
 * handle's max_batch or more pixels in all than its max_pixels; a ragged handle without a set; an undersized tracked buffer (mbn_alloc's bounds
 * rule: the maps span batch * rows * cols elements, in the ragged form max(dst_offset + rows * cols); regions batch * max_regions records;
 * n_regions_i32 batch elements). MBN_EUNSUPPORTED: a map of 2^31 bytes or more (rows * cols >= 2^29: indices and areas are int32), batch > 65535,
 * max_regions > MBN_COMPONENTS_MAX_REGIONS. A refusal launches nothing. mbn_components_envelope answers the shape part, mbn_components_tile the
 * tile of the first kernel (a seam of the union-find lies at every multiple of it); both and _scratch_bytes (0 for arguments _create refuses) are
 * pure host functions. mbn_components_create: MBN_EINVAL for max_batch < 1 or max_pixels < 1, MBN_EUNSUPPORTED for max_batch > 65535 or
 * max_pixels > 2^34, MBN_ENOMEM when the device has no room. */
#define MBN_COMPONENTS_MAX_REGIONS (1 << 24)
typedef struct mbn_region { int32_t label, area, first_row, first_col, min_row, min_col, max_row, max_col; } mbn_region;
typedef struct mbn_components mbn_components;
int mbn_components_create(mbn_context *ctx, int max_batch, int64_t max_pixels, mbn_components **h);
int mbn_components_destroy(mbn_components *h);
int64_t mbn_components_scratch_bytes(int max_batch, int64_t max_pixels);
int mbn_components_envelope(int batch, int rows, int cols, int classes, int connectivity, int min_area, int max_regions);
int mbn_components_tile(int *tile_rows, int *tile_cols);
int mbn_components_i32(mbn_components *h, void *comp_i32, mbn_region *regions, void *n_regions_i32, void *labels_out_i32, const void *labels_i32,
                       int batch, int rows, int cols, int classes, int connectivity, int min_area, int ignore_label, int max_regions, void *stream);
int mbn_components_ragged_i32(mbn_components *h, mbn_ragged_readout *readout, void *comp_i32, mbn_region *regions, void *n_regions_i32,
                              void *labels_out_i32, const void *labels_i32, int classes, int connectivity, int min_area, int ignore_label,
                              int max_regions, void *stream);
/* Score a segmentation by its regions: panoptic quality (PQ = SQ x RQ, Kirillov et al., CVPR 2019), on the device.
 * Normative (tests/panoptic_ref.py is the numpy form, written as the pair histogram; everything the device writes is an integer, so the result is
 * a function of the input alone: the same bytes at every planning CU count, in both forms, on every run and on graph replay). For one image:
 *   comp_pred [rows][cols] int32: a predicted segment number in [0, n_pred), anything else (-1) is "no segment"; records pred [max_pred].
 *   comp_truth [rows][cols], n_truth, truth [max_truth]: the same for the truth; a truth pixel with comp_truth < 0 is VOID. The records are
 *     mbn_region; only .label and .area are read, and .area must be the number of pixels that carry the segment's number. The calls do not care
 *     who made the maps: two mbn_components_i32 calls are the usual source, whole-class "stuff" segments are as good. A predicted pixel of no
 *     segment still counts in its truth segment's area. With areas that are not the maps' the matches are unspecified (a pair whose union
 *     would fall below its inter never matches, two p may claim one g and either is recorded); nothing faults and nothing outside the tables
 *     is touched.
 *   For a predicted segment p and a truth segment g: inter (p, g) = the pixels in both; void (p) = the pixels of p over void truth;
 *     union (p, g) = area (p) - void (p) + area (g) - inter (p, g).
 *   p and g MATCH iff label (p) == label (g) and 2 * inter > union, in int64 and exact: IoU = 1/2 exactly is no match. A segment has at most
 *     one match on either side (a match needs inter > (area (p) - void (p)) / 2 and inter > area (g) / 2).
 *   A matched p is a TRUE POSITIVE of its class; an unmatched g a FALSE NEGATIVE of its class; an unmatched p a FALSE POSITIVE of its class,
 *     unless 2 * void (p) > area (p): then it is EXCUSED and counts nowhere (a tie is a false positive).
 *   This is pq_compute_single_core of the COCO panoptic API with the crowd rule left out.
 *   pq_u64 [classes][4] = tp, fp, fn, S, row-major on 8 bytes. The calls ADD to it: the caller clears it (mbn_memset) and a dataset accumulates
 *     over many calls. S is the sum over the matches of floor (inter * 2^32 / union) (inter < 2^29: the product fits a uint64). A segment whose
 *     label lies outside [0, classes) adds nothing to pq_u64; it is matched and written to the per-segment outputs like any other.
 * Outputs per image:
 *   scored_i32 [batch]                  1: the image was scored. 0: n_pred > max_pred or n_truth > max_truth: the image adds NOTHING to pq_u64 and
 *                                       none of its other outputs is written. Decided on the device from n_*_i32; a negative n counts as 0. Required.
 *   match_pred_i32 [batch][max_pred]    the matched g; -1 for a false positive; -2 for an excused segment. May be NULL.
 *   match_truth_i32 [batch][max_truth]  the matched p, or -1. May be NULL.
 *   inter_i32 [batch][max_pred]         inter of the match, else 0. May be NULL.
 *   void_i32 [batch][max_pred]          void (p). May be NULL.
 *   Entries are written for i < n only; the rest are untouched.
 *   mbn_panoptic_i32         maps [batch][rows][cols], tables [batch][max_*], n_*_i32 [batch] (device, as mbn_components_i32 wrote them)
 *   mbn_panoptic_ragged_i32  the maps of a ragged set of either item kind: both maps at the labels' dst_offset, nothing between the maps is read;
 *                            the tables are [set batch][max_*]. It keeps the handle's generation rule (a captured launch replayed after a later
 *                            set does nothing) and the next set waits for it
 * Both are a FIXED sequence of six kernels on `stream` (NULL: the context's): clear, vote, candidate, intersect, decide, truth. No host decision,
 * allocation, copy or blocking call: a call may be captured as a linear chain of kernel nodes. The grids are sized from the planning CU count; a
 * unit of the two pixel kernels is MBN_PANOPTIC_CHUNK = 1024 pixels. Calls on one handle share its scratch: they must be ordered on one stream.
 * The handle holds all scratch: mbn_panoptic_scratch_bytes (max_batch, max_slots) = 116 bytes per slot, rounded up to 256, a function of those
 * two numbers only, never of the pixel count. A call needs batch <= max_batch and batch * max (max_pred, max_truth) <= max_slots.
 * mbn_shutdown frees the handles still alive.
 * MBN_EINVAL: a NULL handle, pq_u64, scored_i32, map, table or n_*_i32; a pointer off 4 bytes (pq_u64 off 8); batch, rows, cols, classes,
 * max_pred or max_truth < 1; a request over the handle's limits; a ragged handle without a set or of another context; an undersized tracked
 * buffer (mbn_alloc's bounds rule: the maps span batch * rows * cols elements, in the ragged form max (dst_offset + rows * cols); the tables
 * batch * max_* records or elements; pq_u64 classes * 32 bytes; scored_i32 and n_*_i32 batch elements). MBN_EUNSUPPORTED: rows * cols >= 2^29,
 * batch > 65535, max_pred or max_truth > MBN_COMPONENTS_MAX_REGIONS, classes > MBN_CONFUSION_MAX_CLASSES. A refusal launches nothing.
 * mbn_panoptic_envelope answers the shape part; it and _scratch_bytes (0 for arguments _create refuses) are pure host functions.
 * mbn_panoptic_create: MBN_EINVAL for max_batch < 1 or max_slots < 1, MBN_EUNSUPPORTED for max_batch > 65535 or max_slots > 2^32, MBN_ENOMEM
 * when the device has no room.
 *   mbn_panoptic_metrics   pure C in doubles. For class c with iou = ldexp ((double) S, -32) and den = 2 * tp + fp + fn: a class is PRESENT iff
 *     tp + fp + fn > 0; pq_c = 2 * iou / den, rq_c = 2 * tp / den, sq_c = tp ? iou / tp : 0, each one division; NaN for an absent class.
 *     m: pq, sq, rq = the means over the present classes, summed in ascending class order (0 when there are none); tp, fp, fn = the totals;
 *     classes_present. pq_c, sq_c, rq_c: [classes] or NULL. MBN_EINVAL: NULL pq or m, classes < 1; MBN_EUNSUPPORTED: classes >
 *     MBN_CONFUSION_MAX_CLASSES. */
typedef struct mbn_panoptic_metrics_t {
    double pq, sq, rq, tp, fp, fn;
    int32_t classes_present, reserved;
} mbn_panoptic_metrics_t;
typedef struct mbn_panoptic mbn_panoptic;
int mbn_panoptic_create(mbn_context *ctx, int max_batch, int64_t max_slots, mbn_panoptic **h);
int mbn_panoptic_destroy(mbn_panoptic *h);
int64_t mbn_panoptic_scratch_bytes(int max_batch, int64_t max_slots);
int mbn_panoptic_envelope(int batch, int rows, int cols, int classes, int max_pred, int max_truth);
int mbn_panoptic_metrics(const uint64_t *pq, int classes, mbn_panoptic_metrics_t *m, double *pq_c, double *sq_c, double *rq_c);
int mbn_panoptic_i32(mbn_panoptic *h, void *pq_u64, void *scored_i32, void *match_pred_i32, void *match_truth_i32, void *inter_i32, void *void_i32,
                     const void *comp_pred_i32, const mbn_region *pred, const void *n_pred_i32, int max_pred, const void *comp_truth_i32,
                     const mbn_region *truth, const void *n_truth_i32, int max_truth, int batch, int rows, int cols, int classes, void *stream);
int mbn_panoptic_ragged_i32(mbn_panoptic *h, mbn_ragged_readout *readout, void *pq_u64, void *scored_i32, void *match_pred_i32,
                            void *match_truth_i32, void *inter_i32, void *void_i32, const void *comp_pred_i32, const mbn_region *pred,
                            const void *n_pred_i32, int max_pred, const void *comp_truth_i32, const mbn_region *truth, const void *n_truth_i32,
                            int max_truth, int classes, void *stream);
/* Helpers of the layers above: a uint8 map widened to int32 value for value (255 stays 255, void for classes <= 255), one kernel on `stream`;
 * and the elements the maps of a ragged read-out's last set span, max (dst_offset + rows * cols) (0 without a set). mbn_widen_u8_i32: MBN_EINVAL
 * for a NULL pointer, dst_i32 off 4 bytes, count < 1 or an undersized tracked buffer. */
int mbn_widen_u8_i32(mbn_context *ctx, void *dst_i32, const void *src_u8, int64_t count, void *stream);
int64_t mbn_ragged_readout_span(const mbn_ragged_readout *readout);
/* Score a segmentation at its boundaries: boundary IoU (Cheng et al., CVPR 2021) and the trimap scores of the DeepLab papers, on the device
 * (DESIGN.md 7d.6). Both rest on the DEPTH of a pixel: its Chebyshev distance to the nearest pixel that carries another value. The arithmetic is
 * integer: every result is pinned bit for bit at every planning CU count and on graph replay. Normative (tests/boundary_ref.py is the numpy form):
 *   DEPTH. For one map L [rows][cols], a half-width d >= 1 and edge in {0, 1}, D (r, c) is the smallest max (|dr|, |dc|) >= 1 for which pixel
 *     (r + dr, c + dc) lies inside the map and its value differs from L (r, c), or edge = 1 and that pixel lies outside the map; capped at d + 1.
 *     Values are compared as stored: an int32 as an int32, a uint8 zero-extended. 255, negative values and an ignore_label are values like any
 *     other: a void or abstained pixel is a contour for its neighbours and has a depth itself. A pixel is IN THE BAND iff D <= d. This is d
 *     erosions with a 3 x 3 element, per value. edge = 1 is the official boundary IoU (the image frame is a contour); edge = 0 is what trimap
 *     users want for classes that touch the frame.
 *   HALF-WIDTH. mbn_boundary_d (rows, cols, ratio) = ratio * sqrt ((double) rows * rows + (double) cols * cols) rounded to nearest, ties to even
 *     (nearbyint under the default rounding mode; the int (round (...)) of the official Python), at least 1: the RETURN VALUE (a status is negative).
 *     375 x 500 at 0.02 gives 12, 224 x 224 gives 6. MBN_EINVAL: rows or cols < 1, a ratio not in (0, 1] (NaN included); MBN_EUNSUPPORTED: the
 *     result exceeds MBN_BOUNDARY_MAX_D.
 *   SCORE. For truth t, prediction p, their depths Dt and Dp (same d, same edge) and classes = C:
 *     trimap_u64 [C + 1][C + 1] has the layout and the row and column rules of mbn_confusion_i32 (void row, abstained column). Every pixel with
 *       Dt <= d adds 1 to its cell, no other pixel adds anything: mbn_confusion_metrics of it yields the trimap pixel accuracy, mIoU and the rest.
 *     biou_u64 [C][3]: [c][0] counts the pixels with t == c and Dt <= d; [c][1] those with p == c, Dp <= d and t valid (inside [0, C): a
 *       prediction over void truth is not scored); [c][2] those with t == c, p == c, Dt <= d and Dp <= d.
 *     Both tables are ADDED TO: the caller clears them and a dataset accumulates over many calls. Either may be NULL, not both.
 *   mbn_boundary_depth          depth_u8 [batch][rows][cols] = min (D, d + 1) of map [batch][rows][cols], elem_bytes 1 (uint8) or 4 (int32)
 *   mbn_boundary_depth_ragged   the same over the maps of a ragged set of either item kind (the items' first 16 bytes): depth_u8 and map use the
 *                               labels' dst_offset in ELEMENTS; nothing between the maps is read or written
 *   mbn_boundary_score_i32      labels_i32 and truth (truth_bytes 1 or 4) [batch][rows][cols]. FUSED: both depths are formed in LDS and never
 *                               reach memory
 *   mbn_boundary_score_ragged_i32  the same over a ragged set; truth at the labels' element offsets
 *   Half-width of the ragged forms: d_items_i32 == NULL: d holds for every item. Otherwise d_items_i32 is a DEVICE array [set batch] of int32, one
 *     half-width per item, and d is ignored. The kernel CLAMPS an entry into [1, MBN_BOUNDARY_MAX_D]: the host cannot see a device array without
 *     a copy, and these calls make none. mbn_boundary_d_items (readout, ratio, d_host) is the way to produce that array: pure host, it fills
 *     d_host [set batch] from the handle's pinned items with mbn_boundary_d and answers its refusals (MBN_EINVAL also for a handle without a set).
 * Each of the four device calls is ONE kernel, asynchronous on `stream` (NULL: the context's), capturable as one kernel node; no handle of its
 * own, no scratch, no host copy; a persistent grid sized from the planning CU count; the ragged forms keep the handle's generation rule (a
 * captured launch replayed after a later set does nothing) and the next set waits for them. int32 maps may be any pointers on 4 bytes, uint8 maps
 * and depth_u8 any byte pointers; nothing outside the maps is read.
 * MBN_EINVAL: a NULL pointer (both tables NULL); a table off 8 bytes, an int32 map off 4; batch, rows, cols or classes < 1; d < 1 (without
 * d_items_i32); edge not 0 or 1; elem_bytes or truth_bytes not 1 or 4; d_items_i32 off 4 bytes; depth_u8 overlapping map; a handle without a
 * set; an undersized tracked buffer (mbn_alloc's bounds rule: the maps span batch * rows * cols elements, in the ragged form
 * max (dst_offset + rows * cols); trimap (C + 1)^2 * 8 bytes, biou C * 24 bytes, d_items_i32 4 bytes per item). MBN_EUNSUPPORTED:
 * d > MBN_BOUNDARY_MAX_D, classes > MBN_CONFUSION_MAX_CLASSES, rows * cols >= 2^29, batch > 65535. A refusal launches nothing.
 * mbn_boundary_envelope answers the shape part (classes = 1 for the depth calls). mbn_boundary_tile gives the tile and the LDS bytes a workgroup of
 * the score kernel takes at this d (the depth kernel takes less than half): a seam lies at every multiple of the tile; lds_bytes is monotone in d and at
 * most 160 KiB. The ragged forms with d_items_i32 take what d = MBN_BOUNDARY_MAX_D takes. Pure host functions.
 *   mbn_boundary_metrics   pure C in doubles. n = biou, C = classes. For class c: den = n[c][0] + n[c][1] - n[c][2]; a class is PRESENT iff den > 0;
 *     iou[c] = n[c][2] / den, NaN for an absent class; boundary_miou = the mean over the present classes in ascending class order (0 when there
 *     are none); truth_band_pixels = sum of n[c][0], pred_band_pixels = sum of n[c][1]. Every ratio is one division of exact integers. iou:
 *     [classes] or NULL. MBN_EINVAL: NULL biou or m, classes < 1; MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES. */
#define MBN_BOUNDARY_MAX_D 64
typedef struct mbn_boundary_metrics_t {
    double boundary_miou, truth_band_pixels, pred_band_pixels;
    int32_t classes_present, reserved;
} mbn_boundary_metrics_t;
int mbn_boundary_d(int rows, int cols, double ratio);
int mbn_boundary_d_items(mbn_ragged_readout *readout, double ratio, int32_t *d_host);
int mbn_boundary_envelope(int elem_bytes, int classes, int batch, int rows, int cols, int d, int edge);
int mbn_boundary_tile(int d, int *tile_rows, int *tile_cols, int *lds_bytes);
int mbn_boundary_metrics(const uint64_t *biou, int classes, mbn_boundary_metrics_t *m, double *iou);
int mbn_boundary_depth(mbn_context *ctx, void *depth_u8, const void *map, int elem_bytes, int batch, int rows, int cols, int d, int edge,
                       void *stream);
int mbn_boundary_depth_ragged(mbn_ragged_readout *readout, void *depth_u8, const void *map, int elem_bytes, int d, const void *d_items_i32, int edge,
                              void *stream);
int mbn_boundary_score_i32(mbn_context *ctx, void *trimap_u64, void *biou_u64, const void *labels_i32, const void *truth, int truth_bytes,
                           int classes, int batch, int rows, int cols, int d, int edge, void *stream);
int mbn_boundary_score_ragged_i32(mbn_ragged_readout *readout, void *trimap_u64, void *biou_u64, const void *labels_i32, const void *truth,
                                  int truth_bytes, int classes, int d, const void *d_items_i32, int edge, void *stream);
/* Score a segmentation by surface distance: Hausdorff distance (HD), its percentile (HD95), the average symmetric surface distance (ASSD) and the
 * normalized surface Dice (NSD) at a tolerance, on the device. How far a predicted contour lies from the true one, in pixels.
 * Squared Euclidean distances between pixels are integers and both roots below are formed exactly, so every result is pinned bit for bit at every
 * planning CU count and on graph replay. Normative (tests/surface_ref.py is the numpy form), per map and per class c in [0, classes):
 *   CONTOUR. The contour of c in a map M is the set of pixels with M (p) == c whose mbn_boundary_depth is 1: the pixel has an 8-neighbour inside
 *     the map with another value, or edge = 1 and it lies on the map's frame. Values outside [0, classes) (void truth, abstained labels) are
 *     "another value": they make their neighbours contour and form no class of their own. Values are compared as stored (a uint8 zero-extended).
 *   DIRECTIONS. 0 is predicted -> truth, 1 is truth -> predicted. A contour pixel p of c in the source map is a QUERY; d2 (p) is the minimum of
 *     drow^2 + dcol^2 over the contour pixels of c in the OTHER map of the same image: exact, uncapped, an integer. When c has no contour in the
 *     other map of that image, p is UNMATCHED.
 *   TABLE. surf_u64 [classes][2][MBN_SURFACE_HEAD + bins], row-major on 8 bytes, ADDED TO: the caller clears it (mbn_memset) and a dataset
 *     accumulates over many calls. Per class and direction:
 *       [0] n: all queries;   [1] unmatched;   [2] max_d2 over the matched queries, a 64-bit atomic MAX (a larger value already there stays);
 *       [3] sum256: the sum of isqrt (d2 << 16) = floor (256 d) over the matched queries;
 *       [4 + t], t < bins - 1: the matched queries with ceil (sqrt (d2)) == t (the smallest integer t with t * t >= d2);
 *       [4 + bins - 1]: those with ceil (sqrt (d2)) >= bins - 1 (the OVERFLOW bin).
 *     With ceil, the cumulative count up to an integer tau is exactly the number of matched queries with d <= tau.
 *   dist2_u32 (optional, NULL: not written), at the labels' element offsets, direction 0 only: d2 of a matched query, 0xFFFFFFFE for an unmatched
 *     one, 0xFFFFFFFF for a pixel that is no query. Nothing outside the maps is written. It must not overlap labels_i32 or truth.
 *   mbn_surface_score_i32         labels_i32 and truth (truth_bytes 1 or 4) [batch][rows][cols]
 *   mbn_surface_score_ragged_i32  the same over the maps of a ragged set of either item kind (the items' first 16 bytes): truth and dist2_u32 at
 *                                 the labels' dst_offset in ELEMENTS; nothing between the maps is read or written. It keeps the handle's
 *                                 generation rule (a captured launch replayed after a later set adds nothing) and the next set waits for it
 * Both are a FIXED sequence of three kernels on `stream` (NULL: the context's): clear, contour, search. No host decision, allocation, copy to the
 * host or blocking call: a call may be captured as a linear chain of kernel nodes. The grids are sized from the planning CU count; a unit of the
 * two pixel kernels is MBN_SURFACE_UNIT consecutive pixels of one map (mbn_surface_tile: a seam lies at every multiple of it in row-major pixel
 * order, and between the 64-pixel shares of its waves). The search is not capped: a query far from its match reads every ring between them
 * (profiles/LOG.md, "Surface distance", has the cost). Calls on one handle share its scratch: they must be ordered on one stream.
 * The handle holds all scratch: mbn_surface_scratch_bytes (max_batch, max_pixels, max_classes) = 8 bytes per pixel (two int32 contour maps) + 8
 * bytes per image and class (the presence table), rounded up to 256. A call needs batch <= max_batch, its pixels in all <= max_pixels and
 * classes <= max_classes. mbn_shutdown frees the handles still alive. int32 maps and dist2_u32 may be any pointers on 4 bytes, a uint8 truth any.
 * MBN_EINVAL: a NULL handle, table, labels or truth; a table off 8 bytes; labels, an int32 truth or dist2_u32 off 4; classes < 1; bins < 2; batch,
 * rows or cols < 1; edge not 0 or 1; truth_bytes not 1 or 4; dist2_u32 overlapping an input; a ragged handle without a set or of another
 * context; an undersized tracked buffer (mbn_alloc's bounds rule, interior pointers included: the maps span batch * rows * cols elements, in the
 * ragged form max (dst_offset + rows * cols); the table classes * 2 * (4 + bins) * 8 bytes; last_error names "surface table", "surface labels",
 * "surface truth" or "surface dist2"). MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES, bins > MBN_SURFACE_MAX_BINS, rows or cols > 32767
 * (so that d2 < 2^31), rows * cols >= 2^29, batch > 65535, anything over what the handle was created for. MBN_EINVAL goes first; a refusal launches
 * nothing. mbn_surface_envelope answers the shape part; it, _tile and _scratch_bytes (0 for arguments _create refuses) are pure host functions.
 * mbn_surface_create: MBN_EINVAL for max_batch, max_pixels or max_classes < 1, MBN_EUNSUPPORTED for max_batch > 65535, max_pixels > 2^34 or
 * max_classes > MBN_CONFUSION_MAX_CLASSES, MBN_ENOMEM when the device has no room.
 *   mbn_surface_metrics   pure C in doubles. The pixels of all images and calls POOL in the table: every score is a MICRO average over the
 *     dataset's contour pixels, not a mean of per-image scores. Per class, with k the direction: matched_k = n_k - unmatched_k; the class is
 *     PRESENT iff n_0 + n_1 > 0 and MEASURABLE iff matched_0 > 0 and matched_1 > 0. cum_k (t) = the sum of bins 0..t.
 *       hd   = sqrt (max (max_d2_0, max_d2_1))
 *       hdp  = the larger over k of the smallest t with cum_k (t) >= ceil (percentile / 100.0 * matched_k), formed in double: whole pixels,
 *              rounded up; when that t is the overflow bin the class counts in m.saturated and hdp = bins - 1 is a lower bound
 *       assd = (sum256_0 + sum256_1) / 256.0 / (matched_0 + matched_1): within 1/256 pixel below the true mean
 *       nsd  = (cum_0 (tolerance) + cum_1 (tolerance)) / (n_0 + n_1): unmatched queries count in the denominator
 *     hd, hdp and assd are NaN for a class that is not measurable, nsd for one that is not present. m: hd, hdp, assd = the means over the
 *     measurable classes, nsd = the mean over the present ones, summed in ascending class order (0 when there are none); n and unmatched = the
 *     totals over classes and directions; classes_present, classes_measurable, saturated. hd, hdp, assd, nsd: [classes] or NULL.
 *     MBN_EINVAL: NULL surf or m, classes < 1, bins < 2, tolerance outside [0, bins - 2], percentile outside (0, 100] (NaN included);
 *     MBN_EUNSUPPORTED: classes > MBN_CONFUSION_MAX_CLASSES, bins > MBN_SURFACE_MAX_BINS. */
#define MBN_SURFACE_HEAD 4
#define MBN_SURFACE_MAX_BINS 4096
#define MBN_SURFACE_UNIT 256
typedef struct mbn_surface_metrics_t {
    double hd, hdp, assd, nsd, n, unmatched;
    int32_t classes_present, classes_measurable, saturated, reserved;
} mbn_surface_metrics_t;
typedef struct mbn_surface mbn_surface;
int mbn_surface_create(mbn_context *ctx, int max_batch, int64_t max_pixels, int max_classes, mbn_surface **h);
int mbn_surface_destroy(mbn_surface *h);
int64_t mbn_surface_scratch_bytes(int max_batch, int64_t max_pixels, int max_classes);
int mbn_surface_envelope(int truth_bytes, int classes, int bins, int batch, int rows, int cols, int edge);
int mbn_surface_tile(int *unit_pixels, int *wave_pixels);
int mbn_surface_metrics(const uint64_t *surf, int classes, int bins, int tolerance, double percentile, mbn_surface_metrics_t *m, double *hd,
                        double *hdp, double *assd, double *nsd);
int mbn_surface_score_i32(mbn_surface *h, void *surf_u64, void *dist2_u32, const void *labels_i32, const void *truth, int truth_bytes, int classes,
                          int bins, int batch, int rows, int cols, int edge, void *stream);
int mbn_surface_score_ragged_i32(mbn_surface *h, mbn_ragged_readout *readout, void *surf_u64, void *dist2_u32, const void *labels_i32,
                                 const void *truth, int truth_bytes, int classes, int bins, int edge, void *stream);
/* The classifier tail of the sequence as one call (MobileNet.c:2601-2792): global average pool (kernel.cl:116) ->
 * FC = pointwise with rows = cols = 1 (kernel.cl:94; bias, no ReLU: B15) -> softmax + top-k. fp32 NHWC,
 * in [batch][rows][cols][channels], fc_w [classes][channels], fc_bias [classes] or NULL; pooled_scratch
 * [batch][channels] and logits_scratch [batch][classes] are caller-provided device buffers (the logits stay readable
 * there). Three launches on `stream`. */
int mbn_classifier_tail(mbn_context *ctx, void *topk_idx_i32, void *topk_prob_f32, void *probs, void *logits_scratch,
                        void *pooled_scratch, const void *in, const void *fc_w, const void *fc_bias, int batch, int rows,
                        int cols, int channels, int classes, int k, void *stream);
/* Global average pool + FC as ONE launch for 1...4 images (MobileNet.c:2601-2739: the `pool` launch, kernel.cl:116, and the
 * `pointwise` launch with rows = cols = 1, kernel.cl:94; bias, no ReLU). fp32 NHWC in [batch][rows][cols][channels] (the window
 * is the whole map), fc_w [classes][channels], fc_bias [classes] or NULL, logits [batch][classes]. The pooled values are those of
 * mbn_pool bit for bit; the FC sums 64-channel slices in a fixed order (no float atomics): the result of an image does not depend
 * on the batch it is in. `workspace`: mbn_pool_fc_workspace_bytes(channels, classes) bytes of device memory, ZEROED ONCE by the
 * caller (mbn_memset) and then reused launch after launch on one stream at a time. MBN_EUNSUPPORTED for batch > 4 or channels
 * not a multiple of 64 (the caller then uses mbn_pool + mbn_pointwise). */
size_t mbn_pool_fc_workspace_bytes(int channels, int classes);
int mbn_pool_fc(mbn_context *ctx, void *logits, const void *in, const void *fc_w, const void *fc_bias, int batch, int rows, int cols,
                int channels, int classes, void *workspace, size_t workspace_bytes, void *stream);
/* The WHOLE classifier tail as ONE launch for 1...4 images (SURVEY 8f-3 as written; MobileNet.c:2601-2792: the `pool` launch, the FC
 * `pointwise` launch with its blocking read-back of 1000 logits, the host softmax loop :2771-2779 and the host arg-max :2781-2792): global
 * average pool -> FC + bias -> softmax -> top-k, results identical to mbn_pool_fc followed by mbn_softmax_topk_f32 bit for bit. The class
 * range that finishes last (a second arrival counter in the workspace) reads the complete logits back and normalises / ranks them. Same
 * workspace and envelope as mbn_pool_fc, plus classes <= 1024; `logits` [batch][classes] stay readable, `probs` may be NULL.
 * Measured on MI355X (profiles/r04/h_classifier_tail_one_launch.txt): see there — at 1...4 images the tail is launch-latency bound and the
 * one launch is offered as an option, not taken by default. */
int mbn_classifier_tail_fused(mbn_context *ctx, void *topk_idx_i32, void *topk_prob_f32, void *probs, void *logits, const void *in, const void *fc_w,
                              const void *fc_bias, int batch, int rows, int cols, int channels, int classes, int k, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Input front-end on device: uint8 HWC [N][rows][cols][3] -> fp32 NHWC x*scale+bias
 * (Keras MobileNet preprocessing is scale=1/127.5, bias=-1). */
int mbn_normalize_u8_to_f32(mbn_context *ctx, void *out_f32, const void *in_u8, size_t count, float scale,
                            float bias, void *stream);

/* Resize front-end: images of any size -> the plan's rows x cols, on device, in front of the uint8 stem (MBN_IO_IN_U8). What Keras's
 * load_img(target_size=...) does with Pillow: an 8-bit bilinear resize of a box of the source, BYTE FOR BYTE what
 * PIL.Image.resize((out_cols, out_rows), Image.BILINEAR, box=box) returns (tests/golden/resize_pillow.npz records Pillow's own bytes;
 * tests/resize_ref.py restates the arithmetic in numpy). The reference has no counterpart: decode_image (MobileNet.c:49-57) takes 224*224*3 raw bytes.
 * The arithmetic, normative. Source: uint8 HWC [H][W][3]. Box: (left, upper, right, lower), four float32. Output: uint8 [oh][ow][3].
 * Per axis, with in_size, the box edges b0 < b1 (float32) and out_size:
 *     scale = (double)(b1 - b0) / out_size          the subtraction in float32, the division in double
 *     fs = max(scale, 1.0);  support = fs;  ksize = (int)ceil(support) * 2 + 1
 *   and for output index i:
 *     center = (double)b0 + (i + 0.5) * scale
 *     lo = max((int)(center - support + 0.5), 0);  hi = min((int)(center + support + 0.5), in_size)      (the casts truncate toward zero)
 *     n = hi - lo;  tap t < n:  w_t = max(0, 1 - |(t + lo - center + 0.5) / fs|)                           in double
 *     sum = w_0 + w_1 + ... in order;  w_t /= sum when sum != 0;  k_t = (int)(w_t * 4194304.0 + 0.5)       22 fractional bits
 * Two passes, each over all three channels: horizontal first, tmp = clamp((2097152 + sum_t src[lo + t] * k_t) >> 22, 0, 255) ROUNDED TO uint8
 * (int32 sums: the weights are >= 0 and sum to about 2^22), then the vertical pass the same way over tmp. An axis that is neither scaled
 * nor cropped has the weights (2^22, 0): the identity.
 * The filter. What stands above is MBN_FILTER_BILINEAR, the default everywhere and the only filter of every function without `_filter` in its
 * name. The `_filter` functions take one of MBN_FILTER_* (Pillow's own Image.Resampling numbers; any other value: MBN_EINVAL), and give BYTE FOR BYTE
 * what PIL.Image.resize((out_cols, out_rows), filter, box=box) returns (tests/golden/resize_pillow_filters.npz records Pillow 12.2.0's bytes;
 * tests/resize_filters_ref.py restates the arithmetic in numpy).
 * Convolution filters (all but NEAREST) run as above with two changes. The support:
 *     support = S * fs, S = 0.5 (BOX), 1 (BILINEAR, HAMMING), 2 (BICUBIC), 3 (LANCZOS);  ksize = (int)ceil(support) * 2 + 1;  lo, hi with this support
 * and the weight, w_t = f((t + lo - center + 0.5) * (1.0 / fs)): a multiply by the reciprocal, Pillow's own form (BILINEAR keeps the division it
 * has above: its tables are pinned as integers). f in double:
 *     BOX       1 if x > -0.5 && x <= 0.5, else 0
 *     HAMMING   with x = |x|: 1 at 0, 0 for x >= 1, else with x *= M_PI: sin(x) / x * (0.54 + 0.46 * cos(x))
 *     BICUBIC   a = -0.5, with x = |x|: ((a + 2) * x - (a + 3)) * x * x + 1 below 1, (((x - 5) * x + 8) * x - 4) * a below 2, else 0
 *     LANCZOS   sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, otherwise sin(x * M_PI) / (x * M_PI)
 * The sum is taken in order and divides when it is nonzero; k_t = (int)(w_t * 4194304.0 + 0.5) for w_t >= 0 and (int)(w_t * 4194304.0 - 0.5) for
 * w_t < 0. The two passes are unchanged (an int32 sum from 2^21, >> 22 arithmetic, the clamp to [0, 255], the uint8 intermediate): weights
 * may be negative and a row of them need not sum to 2^22. An axis that is neither scaled nor cropped has identity weights under every filter.
 * NEAREST is Pillow's scaled-affine path, no convolution. Per axis
 *     a = (double)(b1 - b0) / out_size  (the subtraction in float32);  xo = (double)b0 + a * 0.5;  for i = 0 .. out_size - 1: index[i] = (int)xo; xo += a
 * with the sum ACCUMULATED: the closed form b0 + a * (i + 0.5) gives other indices (4 of 188 columns for 504 -> 188, 6 of 65 for 1222 -> 65).
 * out[y][x] = src[iy[y]][ix[x]]. For a box inside the image an index never leaves it; it is clamped into the source anyway, for memory safety only.
 * As an axis table NEAREST is ksize 1: first = index, count = 1, weight 2^22.
 * The envelope is the same for every filter: source sides <= 8192, output sides <= 4096, ksize <= 67, and a tile of one output row must fit the
 * kernel's 60 KB of LDS (MBN_EUNSUPPORTED otherwise, from the plan). The largest downscale that leaves per filter (tests/test_resize_filters_cpu.py
 * pins each one step inside and one step outside):
 *     LANCZOS  11x (ksize 67)      BICUBIC  16.5x (ksize 67)      BILINEAR, HAMMING  33x (ksize 67)      NEAREST  any (8192 -> 1)
 *     BOX      66x by its taps (ksize 67) when only the rows shrink; the four staged source rows of a one-row tile bind first when the columns
 *              shrink: 58x with more than 32 output columns (3712 -> 64, not 3776) and 49x on both axes at once (3136 x 3136 -> 64 x 64, not
 *              3200 x 3200), in both kernels; 66x on both axes with at most 32 output columns (a tile of 32 columns stages half as much)
 *   mbn_resize_ksize   ksize of an axis, or a negative status; mbn_resize_ksize_filter likewise (NEAREST: 1)
 *   mbn_resize_taps    the tables of an axis: first[i] = lo, count[i] = n, weights [out_size][ksize] zero padded; returns ksize (>= 3) or a
 *                      negative status. Host code (host/mbn_resize.c; the expressions above are host/mbn_resize_axis.h, compiled for the host
 *                      and for the device); also in libmbn_host.so. mbn_resize_taps_filter likewise (ksize >= 1)
 *   mbn_resize_nearest_index   NEAREST's index [out_size] of an axis; MBN_OK or MBN_EINVAL
 *   mbn_fit_box        the box of a fit mode. MBN_FIT_STRETCH: (0, 0, W, H). MBN_FIT_CROP: the centred box with the output's aspect ratio,
 *                      shrunk by crop_fraction f in (0, 1] (f = 0.875 is the usual "resize to 256, crop 224"); in double
 *                      bw = min(W, H * ow / oh) * f, bh = bw * oh / ow, left = (W - bw) / 2, upper = (H - bh) / 2, each edge then rounded to
 *                      float32 and clamped into the image. 480 x 640 -> 224 x 224, f = 1: (80, 0, 560, 480)
 *                      MBN_FIT_PAD: (0, 0, W, H) again, the whole image being what a letterbox resizes; any other fit: MBN_EINVAL
 *   mbn_fit_pad        the letterbox, normative: PIL.ImageOps.pad(image, (ow, oh), filter, color=fill) of Pillow 12.2.0 (ImageOps.contain, then the
 *                      paste with centering (0.5, 0.5)), byte for byte (tests/golden/resize_pillow_pad.npz records Pillow's bytes). Source H x W,
 *                      canvas oh x ow, everything in double; rint rounds half to EVEN (Python's round):
 *                          im_ratio = W / H;  dest_ratio = ow / oh;  iw = ow;  ih = oh
 *                          if im_ratio != dest_ratio:
 *                              if im_ratio > dest_ratio:  ih = rint(H / W * ow)        the division first, then the product
 *                              else:                      iw = rint(W / H * oh)
 *                          if (iw, ih) == (ow, oh):  x = y = 0
 *                          else if iw != ow:         x = rint((ow - iw) * 0.5);  y = 0
 *                          else:                     x = 0;  y = rint((oh - ih) * 0.5)
 *                      rect = (x, y, iw, ih). The inner image canvas[y .. y + ih)[x .. x + iw) is the resize above of the WHOLE image, box
 *                      (0, 0, W, H), to ih x iw under the handle's filter; every other pixel of the canvas is fill[3] = (R, G, B). 33 x 100 ->
 *                      32 x 32: ih = 11, y = rint(10.5) = 10. iw < 1 or ih < 1 (8192 x 1 -> 32 x 32, where Pillow raises), a non-positive size
 *                      or NULL: MBN_EINVAL. The envelope of a letterbox is the one below applied to (H, W) -> (ih, iw)
 * A box edge below 0 or beyond the image, b1 <= b0, a NaN or a non-positive size: MBN_EINVAL.
 * Device (mbn_u8_resize.hip; the tile body, mbn_u8_resize.h, is the ragged kernel's too): ONE launch runs both passes; the uint8 intermediate
 * lives in LDS and never reaches memory.
 *   mbn_resizer_create  builds both tap tables on the host and uploads them (blocking: here, not in the hot call). box NULL = the whole
 *                       image. Envelope: source sides 1..8192, output sides 1..4096, ksize <= 67 per axis (a downscale up to 32x, any
 *                       upscale); outside: MBN_EUNSUPPORTED, nothing launched
 *   mbn_resize_u8       in [batch][H][W][3] -> out [batch][oh][ow][3], one geometry for the whole batch (1..65535 images, else MBN_EINVAL /
 *                       MBN_EUNSUPPORTED above). Asynchronous on `stream` (NULL = the context's); no host allocation and no blocking call, so
 *                       it may be captured between mbn_graph_begin / _end. ANY byte pointer is taken for `in` and `out` (a source row is
 *                       read 4 bytes at a time from its first 4-byte boundary on, bytewise around it: the same bytes out); no byte outside
 *                       the two tensors is read or written. The mbn_alloc bounds rule above applies: an undersized tracked `in` or `out` is
 *                       MBN_EINVAL and nothing is launched. NULL pointers, batch <= 0: MBN_EINVAL
 *   mbn_resizer_destroy frees the handle (waits for the context's stream); mbn_shutdown frees the handles still alive
 *   mbn_resizer_create_filter   the same under any filter; mbn_resizer_create is its MBN_FILTER_BILINEAR call. The filter belongs to the handle:
 *                       mbn_resize_u8 is the one hot call. The five convolution filters run the same kernel on their own tables; NEAREST has a
 *                       kernel of its own, a gather of 3-byte pixels through the uploaded ix [out_cols], iy [out_rows], under the same contract
 *                       (any byte pointers: dword stores from the first 4-byte boundary of an output row's address on, bytewise around them)
 *   mbn_resizer_create_pad      the letterbox of mbn_fit_pad as a handle: mbn_resize_u8 then takes in [batch][H][W][3] to the CANVAS
 *                       out [batch][out_rows][out_cols][3]. Any filter. Still ONE kernel node and nothing else: the launch that resizes the
 *                       whole image into the rectangle of every canvas carries, per image, the workgroups that fill what lies outside it, so
 *                       the call stays legal inside a capture. The same contract for pointers and bounds; every byte of the canvas is written, the
 *                       border as NEAREST stores (bytewise to the first 4-byte boundary of the address, dwords, a bytewise tail). fill NULL:
 *                       MBN_EINVAL; an empty inner side: MBN_EINVAL; the envelope: mbn_resizer_create's on (H, W) -> (ih, iw)
 *   mbn_fit_view        the rectangle of one VIEW of test-time augmentation (mbn_view, at mbn_resample_ensemble_f32 above): the whole H x W image,
 *                       its aspect kept, inside a canvas scaled by `scale` about the centre of the out_rows x out_cols canvas:
 *                           sc = (int)rint((double)out_cols * (double)scale);   sr = (int)rint((double)out_rows * (double)scale);
 *                           (x, y, iw, ih) = mbn_fit_pad(H, W, sr, sc), moved by ((out_cols - sc) / 2, (out_rows - sr) / 2)      (integer division)
 *                       MBN_EINVAL unless 0 < scale <= 1, sr >= 1, sc >= 1 and mirror is 0 or 1, and whatever mbn_fit_pad answers. scale = 1 is
 *                       mbn_fit_pad's rectangle exactly. The mirror applies to the inner image only: the rectangle is the same with and without it
 *   mbn_resizer_create_view     mbn_resizer_create_pad with the rectangle given instead of derived: the whole image resized to view->ih x view->iw
 *                       under any filter, mirrored left-to-right when view->mirror = 1, at (view->x, view->y) of the canvas, fill elsewhere. Byte
 *                       for byte canvas = Image.new("RGB", (ow, oh), fill); inner = im.resize((iw, ih), filter); inner =
 *                       inner.transpose(FLIP_LEFT_RIGHT) if mirror; canvas.paste(inner, (x, y)). mbn_resize_u8 and mbn_resizer_destroy are
 *                       unchanged; still ONE kernel node. MBN_EINVAL: a NULL view / fill, a rectangle outside the canvas, an empty side, a
 *                       non-zero reserved word, mirror outside 0 / 1; the envelope: mbn_resizer_create's on (H, W) -> (ih, iw). The mirror costs
 *                       no table of its own: a tile forms its columns in reverse order and lands at the mirrored place (NEAREST: the index table
 *                       is uploaded in reverse) */
#define MBN_FIT_STRETCH 0
#define MBN_FIT_CROP    1
#define MBN_FIT_PAD     2
#define MBN_FILTER_NEAREST  0        /* PIL.Image.Resampling's numbers */
#define MBN_FILTER_LANCZOS  1
#define MBN_FILTER_BILINEAR 2
#define MBN_FILTER_BICUBIC  3
#define MBN_FILTER_BOX      4
#define MBN_FILTER_HAMMING  5
int  mbn_resize_ksize(int in_size, float b0, float b1, int out_size);
int  mbn_resize_taps(int in_size, float b0, float b1, int out_size, int32_t *first, int32_t *count, int32_t *weights);
int  mbn_resize_ksize_filter(int filter, int in_size, float b0, float b1, int out_size);
int  mbn_resize_taps_filter(int filter, int in_size, float b0, float b1, int out_size, int32_t *first, int32_t *count, int32_t *weights);
int  mbn_resize_nearest_index(int in_size, float b0, float b1, int out_size, int32_t *index);
int  mbn_fit_box(int in_rows, int in_cols, int out_rows, int out_cols, int fit, float crop_fraction, float box[4]);
int  mbn_fit_pad(int in_rows, int in_cols, int out_rows, int out_cols, int32_t rect[4]);
typedef struct mbn_resizer mbn_resizer;
int  mbn_resizer_create(mbn_context *ctx, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resizer **r);
int  mbn_resizer_create_filter(mbn_context *ctx, int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resizer **r);
int  mbn_resizer_create_pad(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const uint8_t fill[3], mbn_resizer **r);
int  mbn_fit_view(int in_rows, int in_cols, int out_rows, int out_cols, float scale, int mirror, mbn_view *v);
int  mbn_resizer_create_view(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view,
                             const uint8_t fill[3], mbn_resizer **r);
int  mbn_resize_u8(mbn_resizer *r, void *out_u8, const void *in_u8, int batch, void *stream);
int  mbn_resizer_destroy(mbn_resizer *r);
/* Ragged resize (mbn_u8_resize_ragged.hip): ONE launch takes `batch` images, each with its own rows, cols and box, to one common
 * [batch][out_rows][out_cols][3]. The arithmetic is the one above, byte for byte; what differs is where the taps are formed: no table is built on the
 * host and none crosses to the device. The kernel evaluates the expressions above itself (the host's own code, host/mbn_resize_axis.h), in fp64 with the float32 subtraction, truncating casts, the
 * sum in order, a true division and no contraction into fused multiply-adds, per tile, straight into LDS. An image is an
 * mbn_resize_item: src_offset = bytes from the launch's src pointer to its first byte (any value >= 0, any order, two items may share one), rows, cols,
 * and its box (all four edges; the whole image is (0, 0, cols, rows)). Envelope per image: that of mbn_resizer_create.
 *   mbn_ragged_resizer_create   allocates everything once: descriptors of max_batch (1..65535) images on the device and a pinned host copy. The
 *                               handle belongs to the context: mbn_shutdown frees the ones still alive
 *   mbn_ragged_resizer_set      checks every item (MBN_EINVAL: a bad box, a bad size, a negative offset, batch outside 1..max_batch;
 *                               MBN_EUNSUPPORTED: any one item outside the envelope), plans the tiles (per image a few evaluations of lo / hi per
 *                               tile: no table) and enqueues ONE asynchronous copy of the descriptors on `stream`. No allocation. It first WAITS
 *                               for the handle's previous copy and launches, whatever their streams: they read what it overwrites. A set is not
 *                               part of a graph (a capturing `stream`: MBN_EINVAL). A failed set leaves the handle without a batch: a launch
 *                               then answers MBN_EINVAL
 *   mbn_resize_ragged_u8        the launch, asynchronous on `stream`, ordered behind the set by the stream (another stream: the caller orders
 *                               them). No host allocation, no blocking call: it may be captured between mbn_graph_begin / _end as one kernel node;
 *                               a captured launch belongs to the batch set when it was captured, and replayed after another set it does nothing.
 *                               ANY byte pointer for src and out. The mbn_alloc bounds rule applies: src spans max(src_offset + rows * cols * 3)
 *                               bytes, out batch * out_rows * out_cols * 3; an undersized tracked buffer is MBN_EINVAL and nothing is launched. No
 *                               byte outside the images and the output is read or written
 *   mbn_resize_taps_device      the kernel's own tap function for one axis, into int32 DEVICE arrays first [out_size], count [out_size],
 *                               weights [out_size][ksize] (zero padded), on the context's stream: what mbn_resize_taps gives on the host, so the
 *                               device arithmetic is pinned as tables and not only through bytes. Returns ksize or a negative status
 *                               (MBN_EUNSUPPORTED beyond in_size 8192, out_size 4096 or 67 taps)
 *   mbn_ragged_resizer_create_filter   the same handle under a filter (mbn_ragged_resizer_create is its MBN_FILTER_BILINEAR call); _set and the
 *                               launch are unchanged. NEAREST, BOX, BILINEAR and BICUBIC only: their taps are plain fp64 arithmetic, which the
 *                               kernel forms with the host's bits (the reciprocal 1.0 / fs a true division, no contraction). NEAREST is a kernel
 *                               of its own: lane c of a tile forms its column's index with its own chain of dependent fp64 additions from xo_0
 *                               (at most 4095; no cheaper form gives the same bits), likewise the rows. MBN_FILTER_HAMMING and
 *                               MBN_FILTER_LANCZOS answer MBN_EUNSUPPORTED here: their weights need sin / cos bit-equal to the host's libm,
 *                               which device math does not promise, and a nearly-always-equal form is not shipped. Use mbn_resizer_create_filter
 *   mbn_resize_taps_device_filter      mbn_resize_taps_device under one of those four filters (HAMMING, LANCZOS: MBN_EUNSUPPORTED): what
 *                               mbn_resize_taps_filter gives on the host (NEAREST: first = the index, count 1, weight 2^22)
 *   mbn_ragged_resizer_create_pad      the letterbox of mbn_fit_pad for images of different sizes: in ONE launch image i goes to its own rectangle
 *                               of canvas i of out [batch][out_rows][out_cols][3] and the rest of every canvas is `fill`. _set and the launch
 *                               are driven as above, with the same generation, first-set-waits and failed-set rules; an item's box must be the
 *                               whole image (0, 0, cols, rows), else MBN_EINVAL, as is an empty inner side. The same four filters. The inner
 *                               size is the image's own, so its axis geometry, tile counts and the workgroup -> (image, tile) search run on
 *                               96-byte descriptors (mbn_resize_pad_desc, host/mbn_envelope.h); the border is written by extra workgroups of the
 *                               same launch, counted into each image's share of the grid ("Letterbox") */
typedef struct mbn_resize_item { int64_t src_offset; int32_t rows, cols; float box[4]; } mbn_resize_item;   /* 32 bytes */
typedef struct mbn_ragged_resizer mbn_ragged_resizer;
int  mbn_ragged_resizer_create(mbn_context *ctx, int max_batch, int out_rows, int out_cols, mbn_ragged_resizer **r);
int  mbn_ragged_resizer_create_filter(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, mbn_ragged_resizer **r);
int  mbn_ragged_resizer_create_pad(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, const uint8_t fill[3],
                                   mbn_ragged_resizer **r);
int  mbn_resize_taps_device_filter(mbn_context *ctx, int filter, int in_size, float b0, float b1, int out_size, void *first_i32, void *count_i32,
                                   void *weights_i32);
int  mbn_ragged_resizer_set(mbn_ragged_resizer *r, const mbn_resize_item *items, int batch, void *stream);
int  mbn_resize_ragged_u8(mbn_ragged_resizer *r, void *out_u8, const void *src_u8, void *stream);
int  mbn_ragged_resizer_destroy(mbn_ragged_resizer *r);
int  mbn_resize_taps_device(mbn_context *ctx, int in_size, float b0, float b1, int out_size, void *first_i32, void *count_i32, void *weights_i32);

/* fp32 <-> bf16 (round to nearest even) on device; used to build the bf16 copy of the pointwise/FC filters. */
int mbn_convert_f32_to_bf16(mbn_context *ctx, void *dst_bf16, const void *src_f32, size_t count, void *stream);
int mbn_convert_bf16_to_f32(mbn_context *ctx, void *dst_f32, const void *src_bf16, size_t count, void *stream);
/* LAB BUILD ONLY as far as any kernel reads it (mbn_bf16_pw_wide.hip: 196 x 256 tiles with the filter loaded from this image straight
 * into matrix-operand registers — built and measured in round 3, slower than the tiled GEMM, not shipped; profiles/LOG.md). The shipped
 * library accepts MBN_IO_FILT_PACKED and ignores the image; mbn_pack_filter_bf16 answers MBN_EUNSUPPORTED there.
 * Packed image of a bf16 pointwise filter [cout][cin]: the same cout * cin bf16 values in the order
 * [cout / 256][cin / 64][8 waves][4 k16 steps][64 lanes][8], i.e. the B operand of v_mfma_f32_32x32x16_bf16 per 32-column
 * wave, so that a wave's share of a k-tile is four contiguous 1-KB loads. mbn_packed_filter_offset = where the image goes
 * inside the filter buffer (cout * cin * 2 bytes rounded up to 256), 0 when the shape has no packed form (cout % 256 or
 * cin % 64 != 0). mbn_pack_filter_bf16 writes the image from the plain filter at the start of `filter_buf` (which must hold
 * offset + cout * cin * 2 bytes). */
size_t mbn_packed_filter_offset(int cout, int cin);
int mbn_pack_filter_bf16(mbn_context *ctx, void *filter_buf, int cout, int cin, void *stream);

/* ------------------------------------------------------------------ loaders
 * The two reference symbols are kept with their exact signatures (CPU only). They return without
 * touching the destination when the file is missing instead of dereferencing NULL
 * (the reference does not check fopen: MobileNet.c:37,52). */
void readSquezeNetKernel(int *m, int read_size);                        /* MobileNet.c:31 — reads "weights_c.txt" */
int  decode_image(unsigned char frame[], char filename[]);              /* MobileNet.c:49 — raw 224*224*3 bytes from offset 0 */

int  mbn_read_text_weights(const char *path, int *m, int read_size);    /* checked form of readSquezeNetKernel */
int  mbn_read_text_weights_f32(const char *path, float *m, size_t read_size, size_t skip);
int  mbn_read_ppm(const char *path, unsigned char *rgb, int *width, int *height, int max_pixels); /* P6, header skipped (B14) */
int  mbn_write_ppm(const char *path, const unsigned char *rgb, int width, int height);
int  mbn_split_rgb(const unsigned char *hwc, int pixels, unsigned char *r, unsigned char *g,
                   unsigned char *b);                                   /* MobileNet.c:218-238 */
/* MobileNet.c:2771-2792: double softmax over uint8 logits + argmax; *location is 1-based like the reference
 * (and defined — 1 — when class 0 wins, which the reference leaves uninitialised: B11). */
int  mbn_softmax_argmax_u8(const unsigned char *logits, int n, double *probs, int *location, double *maximum);

/* ------------------------------------------------------------- Keras .h5 reader */
typedef struct mbn_h5 mbn_h5;   /* opaque: a memory-mapped HDF5 file */
int  mbn_h5_open(const char *path, mbn_h5 **h5);
int  mbn_h5_close(mbn_h5 *h5);
/* Look up a dataset by absolute path ("/conv1/conv1/kernel:0"; the leading "/model_weights" of a full
 * Keras model file is tried too). On success *data points into the mapping (valid until close),
 * shape[0..*ndim-1] is filled (ndim capacity 8). Only contiguous little-endian float32 datasets. */
int  mbn_h5_get(mbn_h5 *h5, const char *name, int *ndim, int64_t shape[8], const float **data);
/* Enumerate every dataset path in the file, depth-first; cb returns non-zero to stop. */
int  mbn_h5_visit(mbn_h5 *h5, int (*cb)(const char *path, int ndim, const int64_t *shape, void *user),
                  void *user);
/* Minimal writer (weight-format tooling): creates a v0-superblock file with old-style
 * groups and contiguous float32 datasets — the subset the reader and libhdf5 both accept. */
typedef struct mbn_h5_writer mbn_h5_writer;
int  mbn_h5_create(const char *path, mbn_h5_writer **w);
int  mbn_h5_put(mbn_h5_writer *w, const char *name, int ndim, const int64_t *shape, const float *data);
int  mbn_h5_finish(mbn_h5_writer *w);   /* writes the file and frees the writer */

/* ------------------------------------------------------ topology (layer table) */
enum { MBN_L_CONV = 1, MBN_L_DW = 2, MBN_L_PW = 3, MBN_L_POOL = 4, MBN_L_FC = 5 };

typedef struct mbn_layer_desc {
    int32_t index;        /* 1-based reference layer number (1 conv, 2..27 dw/pw, 28 pool, 29 FC) */
    int32_t kind;         /* MBN_L_* */
    int32_t in_rows, in_cols, in_ch;
    int32_t out_rows, out_cols, out_ch;
    int32_t stride;
    int32_t pad_top, pad_left;       /* TF-SAME */
    int32_t dilation;     /* depthwise layers of an output_stride 16 / 8 plan: dilation of the 3x3 filter (2 or 4); 0 = none (readers treat 0 as 1).
                           * It fills what was the padding in front of w_offset: the struct's size (80) and every other offset are unchanged */
    int64_t w_offset;     /* float offset of this layer's filter in the packed blob */
    int64_t w_count;
    int64_t scale_offset; /* float offset of per-channel scale (out_ch floats); -1 = none */
    int64_t shift_offset; /* float offset of per-channel shift / bias; -1 = none */
} mbn_layer_desc;

#define MBN_MAX_LAYERS 32
typedef struct mbn_plan {
    int32_t  n_layers;          /* 29 */
    int32_t  res;               /* input side of a square plan (224, 192, 160, 128 or any multiple of 32); 0 for a non-square plan:
                                 * the input is always layer[0].in_rows x layer[0].in_cols */
    float    alpha;             /* width multiplier */
    int32_t  classes;           /* 1000 */
    int64_t  blob_floats;       /* size of the packed, BN-folded parameter blob */
    int64_t  max_act_floats;    /* largest per-image activation (floats) across layers */
    mbn_layer_desc layer[MBN_MAX_LAYERS];
} mbn_plan;

/* MobileNet.c:13-26 + SURVEY §2.1 table, parameterised: channels = max(8, int(c*alpha)), sizes from res. */
int  mbn_plan_build(float alpha, int res, int classes, mbn_plan *plan);
/* The same for rows x cols images (Keras input_shape = (rows, cols, 3)): every layer's height and width follow their own side, pad_top
 * from the rows, pad_left from the cols, max_act_floats from h * w. Both sides must be multiples of 32 in [32, 4096] (MBN_EUNSUPPORTED /
 * MBN_EINVAL as mbn_plan_build). The blob layout and every offset do not depend on the input size. plan->res = rows when rows == cols
 * (mbn_plan_build(a, r, c) is mbn_plan_build_hw(a, r, r, c), byte for byte), 0 otherwise. */
int  mbn_plan_build_hw(float alpha, int rows, int cols, int classes, mbn_plan *plan);
/* The same with an output stride (the option of TF-slim's mobilenet_v1_base): output_stride = 32 (or 0) is mbn_plan_build_hw byte for byte;
 * 16 or 8 stops subsampling once the map is 1/16 or 1/8 of the input, so layer 27 is a dense feature map for detection / segmentation heads
 * (mbn_net_forward(..., last_layer = 27)). Walk the 13 depthwise layers with current = 2 (conv1's stride) and rate = 1; a layer whose table
 * stride is s runs, if current == output_stride, with stride 1 and dilation `rate`, and then rate *= s; otherwise with stride s, undilated, and
 * then current *= s. A dilated stride-1 layer pads D on each side (SAME with the window 2 D + 1) and keeps the map size. 1.0x224: 16 turns
 * layer 24 into stride 1 and dilates layer 26 by 2 (14 x 14 out); 8 turns layers 12 and 24 into stride 1, dilates 14-24 by 2 and 26 by 4 (28 x 28).
 * The blob layout and every offset do not depend on it (trained weights stay valid); max_act_floats follows the larger maps. Any other value:
 * MBN_EINVAL. Dilated layers run as their own launches (no fused kernel takes one) in fp32 and bf16; the I8 mode refuses such a plan. */
int  mbn_plan_build_os(float alpha, int rows, int cols, int classes, int output_stride, mbn_plan *plan);

/* int8 inference mode (MBN_DT_I8). The arithmetic, normative (tests/test_int8_*.py reproduce it bit for bit):
 *   activations  uint8 NHWC, zero point 0, real value = q * s_l with one fp32 scale per layer. Every conv / depthwise / pointwise layer
 *                ends in ReLU6, so s_l = min(6, clip_l) / 255 (default clip_l = 6) and clamping q to [0, 255] IS the ReLU6. The pool
 *                output keeps its input's scale.
 *   weights      int8, symmetric, one scale per output channel (pointwise / FC: per row [Cout][Cin]; depthwise: per channel over its 9
 *                taps). absmax = max |w| of the channel; inv = 127.0f / absmax (float); q = clamp(rintf(w * inv), -127, 127) (float
 *                product, round half to even); s_w = absmax / 127 (double). An all-zero channel: q = 0, s_w = 1.
 *                conv1 keeps its fp32 filter and fp32 arithmetic; only its output is quantized.
 *   requantize   per output channel c, in double, rounded once to float:
 *                  mult[c] = (float)(s_w[c] * s_in * bn_scale[c] / s_out),  bias[c] = (float)(bn_shift[c] / s_out)
 *                (conv1: s_w * s_in = 1; FC: bn_scale = 1, s_out = 1). The kernel forms acc = sum x * w exactly in int32 and
 *                  y = fadd_rn(fmul_rn((float)acc, mult[c]), bias[c])        (no FMA: numpy float32 reproduces it)
 *                uint8 outputs store clamp(rintf(y), 0, 255); the FC (MBN_IO_OUT_F32) stores y, the fp32 logit. conv1's acc is its fp32
 *                convolution sum instead. |acc| <= 255 * 127 * K < 2^31 needs K <= 65536: a larger K answers MBN_EUNSUPPORTED.
 *   pool         global average: q = clamp(rintf(fmul_rn((float)sum, 1.0f / (rows * cols))), 0, 255), sum exact.
 * C-ABI in this mode (ext->dtype = MBN_DT_I8, layout NHWC only; NCHW answers MBN_EUNSUPPORTED): ext->scale / ext->shift are mult / bias
 * above, both required except for the pool; filters are int8 (1 byte) in the layouts of the fp32 mode, conv1's stays fp32 [3][3][cin][C];
 * activations are 1 byte; mbn_convolute reads the fp32 image or, with MBN_IO_IN_U8, the raw uint8 image (x/127.5 - 1 at load).
 * mbn_pointwise with MBN_IO_OUT_F32 writes fp32 (the FC) and requires MBN_ACT_NONE; MBN_ACT_NONE is accepted only there, every uint8
 * output clamps to [0, 255].
 * conv1: 3x3, 3 input channels. Depthwise: 3x3, stride 1 or 2. Channel counts (conv1 / depthwise / pointwise outputs, pointwise / pool inputs) must be multiples
 * of 8, otherwise MBN_EUNSUPPORTED. The fused entry points (stem, blocks, resident, pool + FC) have no I8 form.
 * No dilation: mbn_depthwise with ext->dilation > 1 answers MBN_EUNSUPPORTED in this mode (and in LITERAL), and mbn_quantize_i8 /
 * mbn_net_set_dtype(net, MBN_DT_I8) answer MBN_EUNSUPPORTED for a plan with a dilated layer (mbn_plan_build_os with output stride 16 or 8). */
typedef struct mbn_i8_layer {
    int64_t w_offset;        /* byte offset of the int8 filter in the i8 blob (element order of the fp32 blob's filter); -1: conv1 keeps fp32, pool */
    int64_t mult_offset;     /* byte offset of out_ch fp32 multipliers; -1 for pool */
    int64_t bias_offset;     /* byte offset of out_ch fp32 offsets;     -1 for pool */
    float   in_scale, out_scale;   /* activation scales; FC out_scale = 0 (fp32 logits); conv1 in_scale = 1 (fp32 image) */
} mbn_i8_layer;
typedef struct mbn_i8_params { int32_t n_layers; int64_t blob_bytes; mbn_i8_layer layer[MBN_MAX_LAYERS]; } mbn_i8_params;

/* Quantize a plan's fp32 blob (BN folded) for the I8 mode. act_scales: plan->n_layers entries s_l (NULL = the defaults 6/255; pool and
 * FC entries are ignored; each used one must be finite and > 0). Fills *p; i8_blob NULL = fill *p only, else p->blob_bytes bytes are
 * written there. Layout: per layer, in order, [int8 filter][mult (out_ch fp32)][bias (out_ch fp32)], each segment 256-byte aligned;
 * conv1 has no filter segment (its fp32 filter is read from the fp32 blob at plan->layer[0].w_offset), the pool has none at all.
 * MBN_EUNSUPPORTED for a plan whose channel counts the I8 kernels do not cover or that has a dilated layer (see above). Host code only: also in libmbn_host.so. */
int  mbn_quantize_i8(const mbn_plan *plan, const float *blob, const float *act_scales, mbn_i8_params *p, void *i8_blob);

/* Host-side packed weights: one contiguous fp32 blob (this is what is broadcast over RCCL). */
typedef struct mbn_weights {
    mbn_plan plan;
    float   *blob;        /* plan.blob_floats floats, malloc'd; free with mbn_weights_free */
} mbn_weights;

/* Read a Keras-applications MobileNet-V1 weights file: finds conv1 / conv_dw_i / conv_pw_i / *_bn /
 * conv_preds by name, checks every shape against the plan, folds BatchNorm (eps = 1e-3) into per-channel
 * scale/shift, repacks HWIO -> kernel layouts (pointwise -> [Cout][Cin]). alpha <= 0 => infer from conv1. */
int  mbn_weights_from_h5(const char *path, float alpha, int res, mbn_weights *w);
/* The same with a rows x cols plan (mbn_plan_build_hw); rows <= 0 => 224, cols <= 0 => rows. The blob is that of any square load. */
int  mbn_weights_from_h5_hw(const char *path, float alpha, int rows, int cols, mbn_weights *w);
/* The same with the plan of mbn_plan_build_os(..., output_stride): the same blob, byte for byte, under a plan with larger final maps. */
int  mbn_weights_from_h5_os(const char *path, float alpha, int rows, int cols, int output_stride, mbn_weights *w);
/* Deterministic synthetic weights: N(0, 2/fan_in) kernels, BN gamma U[.5,1.5], beta N(0,.1),
 * mean N(0,.1), var U[.5,1.5]; written in Keras layout so the same reader path loads them. */
int  mbn_weights_synthetic_h5(const char *path, float alpha, int classes, uint64_t seed);
int  mbn_weights_free(mbn_weights *w);

/* -------------------------------------------- whole-network runner (the C host)
 * Replaces the 29 hand-unrolled per-layer blocks of MobileNet.c:240-2763: same layer order, but
 * activations stay resident in HBM (no per-layer D2H/H2D, MobileNet.c:350,395) and weights are uploaded once. */
typedef struct mbn_net mbn_net;
int  mbn_net_create(mbn_context *ctx, const mbn_weights *w, int max_batch, mbn_net **net);
/* Same, but the packed blob already lives on the device (e.g. received by an RCCL broadcast). The net
 * does not take ownership of dev_blob. */
int  mbn_net_create_from_device_blob(mbn_context *ctx, const mbn_plan *plan, const void *dev_blob,
                                     int max_batch, mbn_net **net);
int  mbn_net_destroy(mbn_net *net);
/* MBN_DT_F32 (default) or MBN_DT_BF16: in bf16 mode the net keeps a bf16 copy of the pointwise/FC filters (made on
 * the device from the fp32 blob), activations are bf16, images stay fp32 [batch][rows][cols][3], logits stay fp32.
 * MBN_DT_I8: the net quantizes the fp32 blob with its current activation scales (mbn_quantize_i8; the device blob is downloaded
 * once for that) and uploads the i8 blob; activations are uint8 (layer_output: 1 byte per element), logits stay fp32. Every layer
 * runs as its own launch (no stem, block, resident or pool + FC fusion: mbn_net_launches lists 29 single layers). */
int  mbn_net_set_dtype(mbn_net *net, int dtype);
/* I8 activation scales s_l (n = plan.n_layers entries; pool / FC entries ignored). Setting them re-quantizes when the net is in I8
 * mode. Default 6/255 everywhere. */
int  mbn_net_set_act_scales_i8(mbn_net *net, const float *scales, int n);
int  mbn_net_get_act_scales_i8(const mbn_net *net, float *scales, int n);
/* Calibration: an fp32 forward of `batch` device images (the net's input format) records every conv / depthwise / pointwise layer's
 * output maximum max_l and sets s_l = min(6, max_l) / 255 (6/255 where max_l = 0); re-quantizes in I8 mode. The dtype and every
 * other setting are left as they were. Synchronous. */
int  mbn_net_calibrate_i8(mbn_net *net, const void *images, int batch);
/* Pipeline every forward over `n` contiguous sub-batches on n streams (1 <= n <= 8; default 1). The HBM-bound
 * depthwise kernels of one sub-batch then overlap the MFMA-bound pointwise kernels of another and fill their tails
 * (fp32 1.0x224 batch 256 with the round-2 kernels: +4.7 % at n = 2, -5 % at n = 3, -3 % at n = 4 — smaller sub-batches
 * quantise the GEMM grids worse; bf16 batch 512: -3 % at n = 2; profiles/r02/k_streams_ab.txt). Sub-batches of fewer
 * than 5 images are not forked. The call still behaves as ONE asynchronous operation on the
 * context's stream: the sub-streams fork from it and join back into it. */
int  mbn_net_set_streams(mbn_net *net, int n);
/* With n > 1 streams: 1 = the caller guarantees that `images` is not being produced by work still pending on the
 * context's stream (e.g. it was uploaded with the blocking mbn_upload, or is a resident benchmark input), so the
 * sub-streams need not wait for the context's stream at the start of a forward. Consecutive forwards then overlap
 * across the step boundary (sub-batch j of step k+1 only waits for sub-batch j of step k); the join into the
 * context's stream is still queued, so mbn_sync / later work on that stream stays ordered after the results. */
int  mbn_net_set_free_running(mbn_net *net, int enabled);
/* 1 = capture the 29 launches of a forward into a hipGraph the first time a (images, logits, batch, last_layer)
 * combination is seen and replay it afterwards (re-captured when any of them changes). For launch-bound batches:
 * measured 0.285 -> see DESIGN.md ms per forward at batch 1. Ignored with more than one stream or in timed forwards. */
int  mbn_net_set_graph(mbn_net *net, int enabled);
/* 1 (default) = run layers 1-3 through mbn_stem_fused when the plan allows it (fp32, alpha = 1, activations not
 * kept, at least 3 layers requested); 0 = always issue the 29 separate layer calls. mbn_net_fused_layers reports how
 * many leading layers the next forward(batch, last_layer) would fuse (0 or 3). */
int  mbn_net_set_fuse_stem(mbn_net *net, int enabled);
/* 1 = the `images` handed to mbn_net_forward / _timed / _classify are raw uint8 HWC [batch][rows][cols][3] (device);
 * layer 1 (or the fused stem) normalises them at load (MBN_IO_IN_U8). 0 (default) = fp32 NHWC, already normalised. */
int  mbn_net_set_input_u8(mbn_net *net, int enabled);
/* Images of any size for a net: src_u8 is [batch][in_rows][in_cols][3] uint8 on the device; the box of `fit` (mbn_fit_box with the plan's
 * input rows x cols; crop_fraction is ignored by MBN_FIT_STRETCH) is resized (resize front-end above) into a staging buffer of the net, on the
 * context's stream, and *images_u8 receives that buffer: [batch][rows][cols][3] uint8, the `images` of mbn_net_forward / _classify /
 * _forward_dense / _segment under mbn_net_set_input_u8(net, 1), valid until the next call. Any dtype, any plan. The net keeps ONE resizer,
 * rebuilt only when (in_rows, in_cols, fit, crop_fraction) changes, and the staging buffer (max_batch x rows x cols x 3 bytes, allocated on the
 * first call, freed by mbn_net_destroy; MBN_ENOMEM leaves the net usable). Changes nothing in any forward path. */
int  mbn_net_resize_input(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, float crop_fraction,
                          void **images_u8);
/* The same for images of DIFFERENT sizes: image i is [rows[i]][cols[i]][3] uint8 at src_u8 + offsets[i] (device; bytes, >= 0, any order). One
 * mbn_fit_box per image against the plan's rows x cols, then ONE ragged launch (mbn_resize_ragged_u8 above) into the same staging buffer. The net keeps
 * one ragged resizer of max_batch images, created on the first call and freed by mbn_net_destroy. Any dtype, any plan; no forward path changes. */
int  mbn_net_resize_inputs(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *rows, const int32_t *cols, int batch, int fit,
                           float crop_fraction, void **images_u8);
/* The filter of mbn_net_resize_input / _inputs and, through them, mbn_net_segment_images: one of MBN_FILTER_* (else MBN_EINVAL; nothing changes).
 * MBN_FILTER_BILINEAR until this is called. The kept resizers are rebuilt on the next call after a change. Under MBN_FILTER_HAMMING / _LANCZOS
 * mbn_net_resize_inputs passes the ragged path's MBN_EUNSUPPORTED on and the net stays usable (mbn_net_resize_input takes every filter). */
int  mbn_net_set_resize_filter(mbn_net *net, int filter);
int  mbn_net_get_resize_filter(const mbn_net *net, int *filter);
/* MBN_FIT_PAD as the `fit` of mbn_net_resize_input / _inputs: the letterbox of mbn_fit_pad into the plan's rows x cols (mbn_resizer_create_pad /
 * mbn_ragged_resizer_create_pad above); crop_fraction is ignored. The border is the net's pad colour, (0, 0, 0) = Pillow's default until
 * mbn_net_set_pad_color is called (a channel outside 0..255: MBN_EINVAL, nothing changes); the kept resizers are rebuilt on the next call after the
 * fit or the colour changed. No forward path changes. mbn_net_segment_to and mbn_net_segment_images stay stretch-only; mbn_net_segment_fit and
 * mbn_net_segment_images_fit below take MBN_FIT_PAD and give the labels of a letterboxed image at its own size (the read-out of the rectangle
 * mbn_fit_pad gives; cutting that rectangle out of mbn_net_segment's label map gives them at the network's resolution only). */
int  mbn_net_set_pad_color(mbn_net *net, int r, int g, int b);
int  mbn_net_get_pad_color(const mbn_net *net, int *r, int *g, int *b);
int  mbn_net_fused_layers(const mbn_net *net, int last_layer, int *count);
/* Fused depthwise->pointwise blocks (mbn_dwpw_fused): bit L of `mask` (L = 1-based number of a depthwise layer) lets
 * layers L and L+1 run as one launch when the plan is fp32, activations are not kept and the shapes are inside the
 * kernel's envelope. Default (until this is called) = MBN_FUSE_BLOCKS_DEFAULT in fp32, MBN_FUSE_BLOCKS_DEFAULT_BF16 in bf16
 * mode: the blocks measured faster fused at batch 256 / 512 on MI355X; 0 = every layer its own launch.
 * Under the fp32 DEFAULT a block is fused only when its launch has at least (compute units / 2) output tiles of 128 x 128
 * (1.0x224: blocks 4-7 from 6 images, blocks 8-11 from 11): below that two shorter launches are faster, and batch 1 runs the
 * stem + 26 single layers; an explicit mask is taken as given. fp32 results are bit-identical either way for calls of 5
 * images and more; for 1..4 images a stand-alone pointwise layer in the few-tile regime takes the split-K kernel
 * (mbn_pointwise), whose summation order differs from the block kernel's in the last bits. */
#define MBN_FUSE_BLOCKS_DEFAULT ((1u << 4) | (1u << 6) | (1u << 8) | (1u << 10))
/* bf16 mode: the matrix work is a sixteenth of fp32's and a block is bound by HBM and the depthwise VALU work: one launch
 * that never writes the depthwise output wins on every block inside the kernel's envelope whose pointwise layer is at
 * most 256 channels wide (one column tile: no depthwise recompute); wider blocks stay two launches under this default
 * and can be forced with an explicit mask. */
#define MBN_FUSE_BLOCKS_DEFAULT_BF16 0x0FFFFFFEu
int  mbn_net_set_fuse_blocks(mbn_net *net, unsigned mask);
int  mbn_net_get_fuse_blocks(const mbn_net *net, unsigned *mask);
/* Back to the state before any mbn_net_set_fuse_blocks call: the measured default of the current dtype WITH its
 * default-only rules (few-tile rule in fp32, one-column-tile rule in bf16), which an explicit mask switches off. */
int  mbn_net_reset_fuse_blocks(mbn_net *net);
/* Pool + FC as one launch (mbn_pool_fc) for calls of 1...4 images in fp32. DEFAULT OFF: measured on MI355X the one launch takes
 * 6.7 us against 1.9 + 2.1 us for the two (the cross-workgroup hand-over of the partial sums is three dependent memory round trips),
 * a forward of one image 0.1371 against 0.1348 ms (profiles/r03/p_pool_fc_one_launch.txt). The pooled values are identical either
 * way; the FC sums in another (fixed) order. */
int  mbn_net_set_fuse_tail(mbn_net *net, int enabled);
/* Runs of equal bf16 blocks on a small map (256 channels, stride 1, at most 10 x 10 pixels: the five 10 x 10 blocks of the 0.5x160 network) as ONE launch with
 * the map resident in LDS (mbn_blocks_resident_bf16), and the 0.5x160 network's last two blocks + pool as another (mbn_tail_resident_bf16). Default 1; 0 = one fused
 * launch per block / one launch per layer as before round 6. bf16 mode only; logits within the bf16 tolerance either way (the arithmetic is the same). */
int  mbn_net_set_fuse_resident(mbn_net *net, int enabled);
/* The launches the next forward(batch, last_layer) issues per (sub-)batch: launch j covers n_layers[j] layers starting
 * at the 1-based layer first_layer[j] (3 = fused stem, 2k = k bf16 blocks resident in LDS (mbn_blocks_resident_bf16), 5 = the
 * resident tail (mbn_tail_resident_bf16), 2 = fused block or fused pool + FC, 1 = single layer). *count = number of launches;
 * the arrays (may be NULL) receive at most `capacity` entries. */
/* (The list and the forward are decided by the same rules, which check the plan, the blob's alignment and the 32-bit bounds
 * of the fused kernels. One case is left: a caller's `logits` / last-layer buffer that is not 16-byte aligned makes a fused
 * call answer MBN_EUNSUPPORTED and the forward issue the layers of that launch separately, more launches than listed.) */
int  mbn_net_launches(const mbn_net *net, int batch, int last_layer, int *first_layer, int *n_layers, int capacity, int *count);
/* images: device fp32 NHWC [batch][res][res][3]; logits: device fp32 [batch][classes]. Asynchronous.
 * last_layer: run layers 1..last_layer only (0 or 29 => all; 5 and 13 = BASELINE configs 1-2), in which
 * case `logits` receives that layer's NHWC activation instead. */
int  mbn_net_forward(mbn_net *net, const void *images, void *logits, int batch, int last_layer);
/* forward + classifier read-out on device: the k <= 8 most probable classes per image (mbn_softmax_topk_f32 over the
 * net's own logits buffer): topk_idx [batch][k] int32, topk_prob [batch][k] fp32, device pointers. What MobileNet.c:2744-2792
 * does with a 1000-byte D2H and a host loop, with 2k values per image to download. */
int  mbn_net_classify(mbn_net *net, const void *images, int batch, int k, void *topk_idx_i32, void *topk_prob_f32);
/* Dense head (fully-convolutional MobileNet-V1; with a trained 1x1 conv_preds a DeepLab-style head): the classifier applied at EVERY pixel of the
 * last feature map instead of its average. For a plan whose last two layers are the pool and the FC (every plan of mbn_plan_build*), F = the layer
 * in front of the pool (27), h x w its output map:
 *   mbn_net_forward_dense  runs layers 1..F exactly as mbn_net_forward(net, images, ., batch, F) does (same launches, streams, dtype rules), skips
 *                          the pool and runs the FC as mbn_pointwise with rows = h, cols = w (MBN_ACT_NONE, the FC's bias, the filter of the
 *                          current mode, MBN_IO_OUT_F32 in bf16 and I8): dense_logits [batch][h][w][classes] fp32 in every mode, on the
 *                          context's stream. On a 1 x 1 map (input 32 x 32 at output stride 32) these are mbn_net_forward's logits bit for bit
 *                          (the pool of one pixel divides by 1) wherever layers 1..F run as the same launches in both calls; in bf16 the
 *                          resident tail, which only the full forward can take, groups its pointwise sums differently: mbn_net_set_fuse_resident).
 *   mbn_net_segment        mbn_net_forward_dense into a scratch buffer of the net, then mbn_upsample_argmax_f32 by factor = input rows / h:
 *                          labels_i32 [batch][rows][cols] int32 and score_f32 (may be NULL) [batch][rows][cols] fp32 at input resolution. The
 *                          factor must be the same for the columns and 8, 16 or 32 (any plan of mbn_plan_build_os), else MBN_EUNSUPPORTED.
 * They keep their buffers in the net (the layer-F activation and, for segment, the dense logits: max_batch x h x w x classes floats), allocated on
 * the first call and freed by mbn_net_destroy; MBN_ENOMEM leaves the net usable. F32, BF16 and I8 (which refuses dilated plans: output stride 32
 * only). The FC and the read-out are not part of a graph captured under mbn_net_set_graph. */
int  mbn_net_forward_dense(mbn_net *net, const void *images, void *dense_logits, int batch);
int  mbn_net_segment(mbn_net *net, const void *images, int batch, void *labels_i32, void *score_f32);
/* Labels at the SOURCE resolution (mbn_resample_argmax_f32 above; the stretch fit only: with a crop the network saw a box of the image and labels
 * for the rest would be invented):
 *   mbn_net_segment_to      mbn_net_forward_dense into the net's dense logits, then mbn_resample_argmax_f32 to out_rows x out_cols: labels_i32 (and
 *                           score_f32, may be NULL) [batch][out_rows][out_cols]. The caller pairs it with mbn_net_resize_input(..., MBN_FIT_STRETCH, ...)
 *                           and the source size. An output below 4 x the map: MBN_EUNSUPPORTED before anything runs
 *   mbn_net_segment_images  the whole path for images of DIFFERENT sizes, as mbn_net_resize_inputs takes them: needs mbn_net_set_input_u8(net, 1)
 *                           (else MBN_EINVAL); mbn_net_resize_inputs with MBN_FIT_STRETCH, mbn_net_forward_dense, then ONE ragged read-out of
 *                           image i to its own rows[i] x cols[i] at labels_i32 + dst_offsets[i] (and score_f32 + dst_offsets[i]; elements). The net
 *                           keeps one ragged read-out handle of max_batch images, created on the first call and freed by mbn_net_destroy. The
 *                           items are checked before anything runs
 * F32, BF16 and I8 (output stride 32 only), any plan of mbn_plan_build_os. A refusal leaves the net usable. */
int  mbn_net_segment_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *score_f32);
int  mbn_net_segment_images(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *rows, const int32_t *cols, int batch,
                            void *labels_i32, const int64_t *dst_offsets, void *score_f32);
/* The same under a fit: labels at the source resolution of images that the network saw stretched OR letterboxed.
 *   mbn_net_segment_fit         uniform sources: src_u8 [batch][in_rows][in_cols][3] uint8 (device). mbn_net_resize_input with `fit`,
 *                               mbn_net_forward_dense, then the read-out to in_rows x in_cols: labels_i32 (and score_f32, may be NULL)
 *                               [batch][in_rows][in_cols]. MBN_FIT_STRETCH: mbn_resample_argmax_f32, the labels of mbn_net_segment_to bit for bit.
 *                               MBN_FIT_PAD: mbn_resample_argmax_window_f32 with mbn_fit_pad's rectangle of the plan's rows x cols, so the border
 *                               gets no label and the image is not distorted. Needs mbn_net_set_input_u8(net, 1), else MBN_EINVAL
 *   mbn_net_segment_images_fit  mbn_net_segment_images with a fit: MBN_FIT_STRETCH issues the plain set and the plain kernel, MBN_FIT_PAD ONE
 *                               window set with every image's own rectangle, then mbn_net_resize_inputs with the fit
 * MBN_FIT_CROP: MBN_EUNSUPPORTED from both, nothing written. Its box has fractional edges (mbn_fit_box), which the integer window above does not
 * express, and the network never saw the rest of the image: labels there would be invented. Any other fit: MBN_EINVAL. The envelope (and, ragged,
 * every item) is checked before the resize and the forward run. */
int  mbn_net_segment_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *score_f32);
int  mbn_net_segment_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *rows, const int32_t *cols, int batch,
                                int fit, void *labels_i32, const int64_t *dst_offsets, void *score_f32);
/* The same three paths with the softmax read-out (mbn_resample_softmax_f32 / _window_f32 / _ragged_f32 above): labels_i32 and prob_f32 (fp32, the
 * shape and offsets of the labels; may be NULL when min_prob > 0) instead of labels and score. Step for step mbn_net_segment_to / _fit /
 * _images_fit: the same checks before anything runs, the same resize, mbn_net_forward_dense, net-owned buffers and ragged handle; min_prob outside
 * [0, 1] or NaN, or NULL prob_f32 with min_prob = 0: MBN_EINVAL; MBN_FIT_CROP: MBN_EUNSUPPORTED, any other fit MBN_EINVAL. Every dtype at output
 * stride 32 (the dense logits are fp32 in every mode), fp32 and bf16 at 16 and 8. At min_prob = 0 the labels are those of the argmax path bit for
 * bit; mbn_net_segment_prob_to at the plan's own input size gives mbn_net_segment's labels (the equivalence stated at mbn_resample_argmax_f32). */
int  mbn_net_segment_prob_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *prob_f32, float min_prob,
                             int ignore_label);
int  mbn_net_segment_prob_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *prob_f32,
                              float min_prob, int ignore_label);
int  mbn_net_segment_prob_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *rows, const int32_t *cols, int batch,
                                     int fit, void *labels_i32, const int64_t *dst_offsets, void *prob_f32, float min_prob, int ignore_label);
/* Segment with runners-up (mbn_resample_topk_f32 above): mbn_net_segment_prob_fit / _prob_images_fit, step for step, with the top-k read-out, in every
 * dtype those serve. labels_i32, prob_f32 and score_f32 are rank-major: [k][batch][in_rows][in_cols] for the uniform call; for the image call rank j
 * of image i at j * plane_stride + dst_offsets[i] (plane_stride in elements, at least max(dst_offsets + rows * cols)). prob_f32 = NULL with
 * min_prob = 0 is the logit form; score_f32 may be NULL. MBN_EINVAL: k outside 1..MBN_TOPK_MAX or above the plan's classes, plane_stride below the
 * span, and what the prob calls refuse; a refused call changes nothing, the read-out set and the record included. Both are recorded as the net's
 * most recent successful segment call: mbn_net_segment_score, _regions, _boundary_* and _panoptic then work on plane 0 (the first batch * in_rows *
 * in_cols elements, or the image call's maps) unchanged, and mbn_net_segment_topk_score on all k planes. */
int  mbn_net_segment_topk_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, int k, void *labels_i32, void *prob_f32,
                              void *score_f32, float min_prob, int ignore_label);
int  mbn_net_segment_topk_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *rows, const int32_t *cols, int batch,
                                     int fit, int k, int64_t plane_stride, void *labels_i32, const int64_t *dst_offsets, void *prob_f32,
                                     void *score_f32, float min_prob, int ignore_label);
/* Test-time augmentation through the letterbox (mbn_resample_ensemble_f32 above): view k is (scales[k], mirrors[k]) of mbn_fit_view into the plan's
 * rows x cols, n_views in 1..MBN_ENSEMBLE_MAX_VIEWS, batch * n_views <= max_batch.
 *   mbn_net_resize_views       src_u8 [batch][in_rows][in_cols][3] uint8 (device) -> the net's staging buffer, view-major: view k's `batch` canvases
 *                              are images k * batch .. of it; *staged receives the buffer, as mbn_net_resize_input reports it. One view resizer
 *                              (mbn_resizer_create_view, the net's filter and pad colour) per (scale, mirror), built or reused from a cache of up
 *                              to MBN_ENSEMBLE_MAX_VIEWS handles keyed on the source size, scale, mirror, filter and colour (a change of filter or
 *                              colour builds new ones; the least recently used one makes room); freed by mbn_net_destroy
 *   mbn_net_segment_views_fit  checks everything first (mbn_net_set_input_u8(net, 1), batch * n_views <= max_batch, every scale and mirror, the
 *                              ensemble's envelope at the source size, the softmax arguments): a refusal writes nothing and leaves the net usable.
 *                              Then mbn_net_resize_views, ONE mbn_net_forward_dense of batch * n_views images and ONE mbn_resample_ensemble_f32 to
 *                              in_rows x in_cols: labels_i32, prob_f32 (may be NULL) and score_f32 (may be NULL) [batch][in_rows][in_cols].
 *                              prob_f32 = NULL with min_prob = 0: the argmax form
 * F32, BF16 and I8 (output stride 32 only), any plan of mbn_plan_build_os: the dense logits are fp32 in all of them. */
int  mbn_net_resize_views(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors,
                          int n_views, void **staged);
int  mbn_net_segment_views_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors,
                               int n_views, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label);
/* Segment by sliding window (mbn_resample_slide_f32 above): the source image is cut into overlapping tile_rows x tile_cols crops, each resized to the
 * plan's rows x cols and run as an image of its own; batch * ny * nx <= max_batch.
 *   mbn_net_resize_tiles   src_u8 [batch][in_rows][in_cols][3] uint8 (device) -> the net's staging buffer, image-major: image b's tile (iy, ix) is
 *                          image b * ny * nx + iy * nx + ix of it; *staged receives the buffer. ONE set on the net's own ragged resizer (the
 *                          stretch handle: a tile is a crop, not a letterbox) and ONE mbn_resize_ragged_u8 launch: the item of that tile is
 *                          { b * in_rows * in_cols * 3, in_rows, in_cols, box = (x, y, x + tile_cols, y + tile_rows) }. The net's filter; the ragged
 *                          path's MBN_EUNSUPPORTED for HAMMING / LANCZOS is passed on. A tile of the plan's own rows x cols comes out as a byte
 *                          copy of the source pixels. MBN_EINVAL / MBN_EUNSUPPORTED: the plan's rules for in_rows x in_cols; MBN_EINVAL: more
 *                          tiles than max_batch
 *   mbn_net_segment_slide  checks everything first (mbn_net_set_input_u8(net, 1), mbn_slide_plan of the arguments, batch * ny * nx <= max_batch,
 *                          the read-out's envelope at the source size, the softmax arguments): a refusal writes nothing and leaves the net
 *                          usable. Then mbn_net_resize_tiles, ONE mbn_net_forward_dense of batch * ny * nx tiles and ONE mbn_resample_slide_f32
 *                          to in_rows x in_cols: labels_i32, prob_f32 (may be NULL) and score_f32 (may be NULL) [batch][in_rows][in_cols].
 *                          prob_f32 = NULL with min_prob = 0: the argmax form
 * F32, BF16 and I8 (output stride 32 only), any plan of mbn_plan_build_os. */
int  mbn_net_resize_tiles(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const mbn_slide *s, void **staged);
int  mbn_net_segment_slide(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int tile_rows, int tile_cols, int stride_rows,
                           int stride_cols, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label);
/* Score the label maps of the net's most recent SUCCESSFUL source-size segment call (mbn_net_segment, _segment_to, _segment_fit, _segment_images,
 * _segment_images_fit, the three _segment_prob_ calls, _segment_views_fit, _segment_slide) against `truth` (uint8 or int32, truth_bytes 1 or 4; "score a
 * segmentation" above): a uniform call is one span of batch * out_rows * out_cols pixels (mbn_confusion_i32), an image call the net's own ragged
 * set (mbn_confusion_ragged_i32: truth at the labels' dst_offsets). classes is the plan's; counts_u64 [classes + 1][classes + 1] is added to.
 * labels_i32 is the buffer that call wrote (or a copy of it). MBN_EINVAL before any such call; a refused segment call leaves the record of the
 * one before in place. Otherwise whatever the confusion call answers. */
int  mbn_net_segment_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *counts_u64);
/* The rank score of the k planes of that same call ("rank score" above; found exactly as mbn_net_segment_score finds it): mbn_topk_rank_i32 for a
 * uniform call, mbn_topk_rank_ragged_i32 on the net's own set for an image call, with the call's k and plane stride and the plan's classes;
 * ranks_u64 [classes + 1][k + 1] is added to. MBN_EINVAL before any segment call and when the last one was not a top-k call. */
int  mbn_net_segment_topk_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *ranks_u64);
/* The calibration table of that same call ("calibration score" above; found exactly as mbn_net_segment_score finds it): mbn_calibration_f32 for a
 * uniform call, mbn_calibration_ragged_f32 on the net's own set for an image call, with the plan's classes; calib_u64 [bins + 1][4] is added to.
 * prob_f32 is the probability map that call wrote (plane 0 of a top-k call), passed by the caller as the labels are: the record does not say
 * whether the last call wrote one. MBN_EINVAL before any segment call. Otherwise whatever the calibration call answers. */
int  mbn_net_segment_calibration(mbn_net *net, const void *labels_i32, const void *prob_f32, const void *truth, int truth_bytes, int bins,
                                 void *calib_u64);
/* The NLL and Brier score of that same call's probabilities ("score the probabilities" above): the dense logits of the most recent successful
 * segment call are still in the net, and this reads them out once more under the geometry that call used, with `truth` (at the labels' element
 * offsets) in the class loop: mbn_resample_nll_f32 for a uniform call (whole map, or the letterbox rectangle of a pad fit; after mbn_net_segment
 * the whole-map call at out = factor x map, whose interpolants are that call's bit for bit), mbn_resample_nll_ragged_f32 on the net's own set for
 * an image call (plane_stride in elements; a uniform call does not read it: its planes are batch * rows * cols apart). The logits are valid until
 * the next segment call (or mbn_net_forward_dense into them). MBN_EINVAL before any segment call; MBN_EUNSUPPORTED after a views or slide call:
 * those logits are several presentations of an image, and averaging them is another probability model. Otherwise whatever the NLL call answers;
 * a refused call leaves the table and the record as they were. */
int  mbn_net_segment_nll(mbn_net *net, const void *truth, int truth_bytes, const float *inv_temps, int temps, void *nll_u64, void *nll_f32,
                         void *brier_f32, int64_t plane_stride);
/* The regions of the label maps of that same call ("regions of a label map" above; found exactly as mbn_net_segment_score finds it): a uniform
 * call is one mbn_components_i32 over [batch][out_rows][out_cols], an image call mbn_components_ragged_i32 on the net's own ragged set. classes is
 * the plan's. The net owns one mbn_components handle, sized for the call on first use, made again when a later call needs more, freed by
 * mbn_net_destroy; MBN_ENOMEM leaves the net usable. MBN_EINVAL before any segment call. Otherwise whatever the components call answers. */
int  mbn_net_segment_regions(mbn_net *net, const void *labels_i32, void *comp_i32, mbn_region *regions, void *n_regions_i32, void *labels_out_i32,
                             int connectivity, int min_area, int ignore_label, int max_regions);
/* The boundary score of the label maps of that same call ("score a segmentation at its boundaries" above; found exactly as mbn_net_segment_score
 * finds it): a uniform call is one mbn_boundary_score_i32 over [batch][out_rows][out_cols], an image call mbn_boundary_score_ragged_i32 on the
 * net's own ragged set. classes is the plan's; trimap_u64 [classes + 1][classes + 1] and biou_u64 [classes][3] are added to, either may be NULL.
 * d > 0 is a fixed half-width and ratio is not read. d == 0 takes ratio: mbn_boundary_d of the output size for a uniform call; for an image call
 * each image's own half-width (mbn_boundary_d_items), uploaded into a net-owned device buffer of max_batch int32 on the context's stream (made on
 * first use, freed by mbn_net_destroy). MBN_EINVAL before any segment call or for d < 0; otherwise whatever mbn_boundary_d and the score call answer.
 * mbn_net_segment_boundary_depth does the same for the band of the labels: depth_u8 at the labels' element offsets (mbn_boundary_depth / _ragged). */
int  mbn_net_segment_boundary_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *trimap_u64, void *biou_u64,
                                    double ratio, int d, int edge);
int  mbn_net_segment_boundary_depth(mbn_net *net, const void *labels_i32, void *depth_u8, double ratio, int d, int edge);
/* The surface-distance score of the label maps of that same call ("score a segmentation by surface distance" above; found exactly as
 * mbn_net_segment_score finds it): a uniform call is one mbn_surface_score_i32, an image call mbn_surface_score_ragged_i32 on the net's own ragged
 * set. classes is the plan's; surf_u64 [classes][2][MBN_SURFACE_HEAD + bins] is added to; dist2_u32 (at the labels' element offsets) may be NULL.
 * The mbn_surface handle is the net's: made on first use for max_batch images, the pixels of the call and the plan's classes, made again when a
 * later call needs more, freed by mbn_net_destroy. MBN_EINVAL before any segment call; otherwise whatever mbn_surface_create and the score call
 * answer. */
int  mbn_net_segment_surface(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, int bins, int edge, void *surf_u64,
                             void *dist2_u32);
/* The panoptic quality of the label maps of that same call ("score a segmentation by its regions" above; found exactly as mbn_net_segment_score
 * finds it) against `truth` (uint8 or int32, truth_bytes 1 or 4; in an image call at the labels' dst_offsets): mbn_components on the labels, the same
 * on the truth (classes the plan's, `connectivity` and `min_area` for both, a label or truth value outside [0, classes) belongs to no segment:
 * the usual 255 is void), then mbn_panoptic: pq_u64 [classes][4] is added to, scored_i32 [batch] says which images were scored: an image with more
 * than the setting's regions on either side is NOT scored, and that is reported here, not hidden. A uint8 truth is first widened to int32 over the
 * flat span of the maps into a net-owned buffer. The net owns the panoptic handle, both segment maps, both tables and counts: made on first use,
 * made again when a later call needs more, freed by mbn_net_destroy; MBN_ENOMEM leaves the net usable. Everything runs on the context's stream with
 * no copy to the host. mbn_net_set_panoptic_regions: the table size of both sides, MBN_NET_PANOPTIC_REGIONS until it is called (MBN_EINVAL below 1,
 * MBN_EUNSUPPORTED above MBN_COMPONENTS_MAX_REGIONS). MBN_EINVAL before any segment call, for a NULL pointer, truth_bytes not 1 or 4 or an int32
 * truth off 4 bytes; otherwise whatever the components and panoptic calls answer. */
#define MBN_NET_PANOPTIC_REGIONS 4096
int  mbn_net_set_panoptic_regions(mbn_net *net, int max_regions);
int  mbn_net_segment_panoptic(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, int connectivity, int min_area, void *pq_u64,
                              void *scored_i32);
/* Per-layer milliseconds of the most recent mbn_net_forward_timed call (hipEvents between layers). */
int  mbn_net_forward_timed(mbn_net *net, const void *images, void *logits, int batch, float *layer_ms,
                           int n_layer_ms);
int  mbn_net_plan(const mbn_net *net, mbn_plan *plan);
/* Device pointer of layer `index`'s output from the most recent forward (valid until the next forward that
 * overwrites the ping-pong buffer; with keep_activations every layer has its own buffer). */
int  mbn_net_set_keep_activations(mbn_net *net, int keep);
int  mbn_net_layer_output(mbn_net *net, int index, void **dptr, size_t *floats_per_image);   /* count: per-image ELEMENTS (fp32, bf16 or uint8) */

/* ------------------------------------------------------------------ multi-GPU (north_star: "batched images
 * shard naturally across the 8 GPUs of one node with an RCCL broadcast of weights over xGMI and no cross-GPU reduction").
 * The reference takes exactly one device (MobileNet.c:155 clGetDeviceIDs(..., 1, &device_id, ...)); this is the form a C
 * host uses to drive all GPUs of a node from one process, one thread per GPU:
 *   mbn_dist_init       one mbn_context per GPU (device_ordinals NULL = 0..n-1) + an RCCL communicator over them
 *                       (ncclCommInitAll; RCCL is bound with dlopen at this call, n_gpus = 1 needs none — with MBN_DIST_FORCE_RCCL=1 in the
 *                       environment one is built for a single GPU too: a rehearsal of the RCCL leg on a one-GPU box);
 *   mbn_dist_context    rank r's context: every other call of this header works on it, from the thread that owns rank r;
 *   mbn_dist_broadcast  dev_ptrs[r] = rank r's device buffer of `bytes` bytes; root's bytes overwrite the others' (one
 *                       grouped ncclBroadcast on the ranks' context streams; returns when all ranks have it). The one
 *                       collective of the path: the packed parameter blob, once, off the timed path;
 *   mbn_dist_sync       mbn_sync on every rank;
 *   mbn_shard_range     the contiguous slice [first, first+count) of `total` images owned by `rank` of `world`: total/world
 *                       each, the first total%world ranks take one more (host arithmetic; also in libmbn_host.so).
 * Contexts are independent, so per-GPU threads need no locking among themselves. */
typedef struct mbn_dist mbn_dist;
int  mbn_dist_init(int n_gpus, const int *device_ordinals, mbn_dist **dist);
int  mbn_dist_size(const mbn_dist *dist, int *n_gpus);
int  mbn_dist_context(mbn_dist *dist, int rank, mbn_context **ctx);
int  mbn_dist_broadcast(mbn_dist *dist, void *const *dev_ptrs, size_t bytes, int root);
int  mbn_dist_sync(mbn_dist *dist);
int  mbn_dist_shutdown(mbn_dist *dist);
const char *mbn_dist_last_error(const mbn_dist *dist);
int  mbn_shard_range(int total, int world, int rank, int *first, int *count);
/* One host thread per rank, for callers that drive several GPUs from one process (`mobilenet --gpus G`): mbn_run_ranks starts
 * n threads, opens a gate once ALL of them exist and runs fn(rank, arg, sync) in each; if a thread cannot be created nobody
 * runs fn and the call returns MBN_ENOMEM (bare pthread_create + pthread_barrier would strand the started ranks in the
 * barrier). Inside fn, mbn_rank_barrier(sync) is a barrier over the n ranks that returns MBN_EDEVICE instead of blocking once
 * any rank has failed (fn returned != MBN_OK, or called mbn_rank_fail). Returns the first failing rank's code;
 * rank_rc (may be NULL) receives every rank's (MBN_EUNSUPPORTED = its job did not run). fail_create_at >= 0 simulates a
 * failed thread creation at that rank (tests). Host code only: also in libmbn_host.so. */
typedef struct mbn_rank_sync mbn_rank_sync;
typedef int (*mbn_rank_fn)(int rank, void *arg, mbn_rank_sync *sync);
int  mbn_run_ranks(int n, mbn_rank_fn fn, void *arg, int fail_create_at, int *rank_rc);
int  mbn_rank_barrier(mbn_rank_sync *sync);
int  mbn_rank_fail(mbn_rank_sync *sync);

const char *mbn_version(void);

/* Process-wide switches. 0 always means "the shipped default". Two kinds:
 *   PRODUCT switches (every build): pw_tile, net_stagger, lit_dot, pw_splitk, pw_emul, pw_emul_static, pw_clock — they select between code
 *     paths the library always contains (a regime a caller or a test wants to force, the opt-in pw_emul arithmetic).
 *   LAB knobs (dw_variant, dw_nseg, pw_stage, conv_variant, misc, pw_ring, pw_xn, dwpw_variant, exp0..2): A/B hooks of the
 *     experiments recorded in profiles/LOG.md. They exist in the lab build only (make lab -> libmbn_lab.so, loaded by the tools with
 *     MBN_LAB=1); the shipped libmbn.so compiles them to zero together with every kernel instantiation only they can reach, and
 *     mbn_tune_set answers MBN_EUNSUPPORTED for them (mbn_tune_get: 0). mbn_lab_build() tells which library this is.
 * Unknown key => MBN_ENOTFOUND.
 *   pw_tile      force a GEMM tile shape of mbn_pointwise (mbn_f32_pw.hip; with pw_emul: mbn_f32_pw_x6.hip); a shape the build does
 *                not contain => MBN_EUNSUPPORTED from the call. 1 also forces the 128-column tile of mbn_dwpw_fused(_bf16);
 *                9 = the short-K resident-filter GEMM (mbn_f32_pw3.hip) wherever eligible, 10 = never (0: where it measured faster; same bits either way)
 *   misc         workgroups per CU of the persistent GEMM grid (1000 = one tile per workgroup); in the split-K kernel 16 / 32 =
 *                force the 16x16 / 32x32 workgroup tile
 *   pw_stage     1 = stage GEMM operands through registers instead of direct-to-LDS loads
 *   conv_variant 1 = generic conv1 kernel; 2 = bf16 fused stem with conv1 on the VALU instead of the bf16 MFMA; 8 = GEMM without the software-pipelined k-loop; 9 = GEMM with the general epilogue;
 *                16 / 32 (with pw_emul): split GEMM without the raised wave priority over the split / with one filter buffer
 *   dw_variant   depthwise: bits 0-1 = output columns per lane, bit 4 = lanes across all channels, bit 5 = bf16 with
 *                4-channel lanes, bit 7 = no raised wave priority
 *   dw_nseg      depthwise: row segments per image
 *   net_stagger  layers between the starts of consecutive sub-batch streams (mbn_net_set_streams)
 *   lit_dot      LITERAL pointwise: 0 = v_mfma_i32_32x32x32_i8 where eligible (no carry quirk, filter fits int8, Cin and Cout >= 16) and measured
 *                faster (K >= 512 or >= 16384 pixels in the call), else the v_dot4_i32_i8 path where eligible; 1 = scalar kernel; 2 = v_dot4 (never
 *                the matrix cores); 3 = the matrix cores wherever eligible. All bit-exact (kernel.cl:94-114)
 *   pw_ring      bf16 pointwise: 0 = streaming ring kernel for K = 64 (shipped), 1 = always the tiled GEMM, 2 = ring wherever eligible
 *   pw_splitk    fp32 pointwise of 1..4 images in the few-tile regime: 0 = split-K kernel (mbn_f32_pw_splitk.hip), 1 = always the
 *                tiled GEMM, 2 = split-K wherever the shape allows (K >= 128, K % 64 == 0), whatever the batch; 16 / 32 = as 2 with
 *                the 16x16 / 32x32 workgroup tile forced (same bits; tests)
 *   pw_emul      fp32 pointwise, OPT-IN arithmetic form (mbn_f32_pw_x6.hip): 0 = v_mfma_f32_32x32x2_f32 (default); 6 or 9 = every fp32
 *                operand split EXACTLY into three bf16 values (x = h + m + l, 24 bits kept) and the product formed from 6 (or all 9)
 *                bf16 x bf16 partial products on v_mfma_f32_32x32x16_bf16 with the fp32 accumulator; fp32 in, fp32 out. The 3 dropped
 *                partial products of 6 are below 2^-24 of the product. Measured error against a float64 product on the network's
 *                layer shapes: equal to or smaller than the fp32 MFMA kernel's (profiles/r02/m_pw_emul.txt); layers 13-27 at
 *                batch 256: 1.41 -> 1.14 ms; with the fused blocks (mbn_dwpw_fused takes mbn_f32_dwpw2_x6.hip for Cin <= 512) and the
 *                pointwise phase of mbn_stem_fused the whole step 89 k -> 109-110 k images/s. Applies to pointwise calls with K % 32 == 0 and at least as many 128x128 tiles as
 *                CUs; everything else takes the default kernels — which form a layer takes therefore depends on the size of the call,
 *                and forward(n)[:k] == forward(k) holds bit for bit only between calls whose layers take the same forms (fused blocks
 *                and stand-alone pairs agree bit for bit under the same value). Each filter pointer gets a pre-split image (6 bytes per
 *                weight) in the context on first use (not inside a hipGraph capture: the unsplit-filter kernel is taken there).
 *                Operand range: the split is exact for 2^-110 <= |x| < 2^127 (measured, profiles/r02/m_pw_emul.txt (19)); in fp32's top
 *                binade h = bf16(x) can round to infinity, below 2^-110 the matrix cores flush the bf16 denormals of the low planes
 *                (2e-6 relative at 2^-115). Post-ReLU6 activations and BN-folded weights are far inside.
 *   pw_emul_static  with pw_emul: 0 = a filter's pre-split image is rewritten by every call that uses it (the filter may change between
 *                calls like any other argument); 1 = the caller's promise that filters are only ever written through mbn_upload /
 *                mbn_memset (or freed through mbn_free): an image is then split once and reused until one of those calls touches its
 *                filter — 13 launches of ~5 us less per forward of the network. bench.py --pw-emul and mobilenet --pw-emul set it
 *                (weights are uploaded once there).
 *   pw_xn        pointwise GEMM tile order: XCD groups along n (0 = by filter size, 1 = single ordering, 2, 4)
 *   dwpw_variant fused block kernel: 0 = shipped choice, 1 = round-1 producer/consumer kernels, 2 = unified-wave kernels,
 *                3 = unified fp32 with the taps read inside the step, 100 + bits = unified with parts switched off
 *   pw_clock     1 = every pw_gemm launch adds the core-clock cycles (s_memtime) and the 100 MHz reference ticks (s_memrealtime) its
 *                first eight workgroups (one per XCD) lived to device counters; mbn_pw_clock_read turns them into the clock the
 *                chip HELD under the fp32 MFMA stream. Off (default): two scalar compares per launch. bench.py sets it for its
 *                untimed profiled steps only, so that `roofline.frac` can be compared across boxes (DVFS: 2.1-2.4 GHz by box;
 *                product switch, every build) */
int  mbn_tune_set(const char *key, int value);
/* Mean core clock (GHz) over the pw_gemm launches recorded since the last reset (tune key pw_clock), and how many launches that was.
 * Waits for the device. reset != 0 clears the counters after reading. No launches recorded => *ghz = 0. The counterpart in the
 * reference is nothing: its only timing is clGetEventProfilingInfo (MobileNet.c:301-305). */
int  mbn_pw_clock_read(mbn_context *ctx, int reset, double *ghz, long long *launches);
int  mbn_lab_build(void);      /* 1 = built with -DMBN_LAB (all A/B variants and knobs), 0 = the shipped library */
int  mbn_tune_get(const char *key, int *value);

#ifdef __cplusplus
}
#endif
#endif /* MBN_H */
