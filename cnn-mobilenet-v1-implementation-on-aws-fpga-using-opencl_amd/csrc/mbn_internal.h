// mbn_internal.h — shared between the C-ABI translation unit and the gfx950 kernel files.
// Not part of the public boundary (that is include/mbn.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "mbn.h"
#include "mbn_envelope.h"

struct mbn_emul_img {
    void *p = nullptr;           // the image (device)
    size_t bytes = 0;            // its size
    size_t src_bytes = 0;        // size of the fp32 filter it was split from (for invalidation by mbn_upload / mbn_memset / mbn_free)
    bool built = false;          // pw_emul_static: the image holds the split of the current filter contents
};

// mbn_resizer_create's handle (mbn_u8_resize.hip): one geometry, its tap tables on the device and the tile the host chose for it
struct mbn_resizer {
    mbn_context *ctx = nullptr;
    int in_rows = 0, in_cols = 0, out_rows = 0, out_cols = 0;
    int filter = MBN_FILTER_BILINEAR;            // MBN_FILTER_*: NEAREST runs the gather kernel on ix [out_cols], iy [out_rows] in `tables`
    mbn_resize_plan_t plan = {};                 // mbn_resize_table_plan; kx, ky = taps per output column / row (the tables' row length)
    void *tables = nullptr;                      // device: fx, cx [out_cols], fy, cy [out_rows], wx [out_cols][kx], wy [out_rows][ky], int32
    // what `out` holds per image: out_rows x out_cols, except under mbn_resizer_create_pad, where out_rows x out_cols is the inner image (ih x iw)
    // at (pad_x, pad_y) of this canvas and `fill` is everywhere else (fill_rows, fill_wgs: mbn_resize_pad_plan_t)
    int canvas_rows = 0, canvas_cols = 0;
    bool pad = false;
    bool mirror = false;                         // mbn_resizer_create_view, mirror = 1: inner column o holds the resize's column out_cols - 1 - o
    int pad_x = 0, pad_y = 0, fill_rows = 0, fill_wgs = 0;
    uint8_t fill[3] = { 0, 0, 0 };
};

// mbn_ragged_resizer_create's handle (mbn_u8_resize_ragged.hip): the descriptors of up to max_batch images, on the device and pinned on the host
struct mbn_ragged_resizer {
    mbn_context *ctx = nullptr;
    int max_batch = 0, out_rows = 0, out_cols = 0, tow = 0, tiles_x = 0;
    int filter = MBN_FILTER_BILINEAR;            // MBN_FILTER_NEAREST, _BOX, _BILINEAR or _BICUBIC: which kernel instantiation a launch takes
    int batch = 0;                               // of the last successful set; 0 = none
    int total_wgs = 0, lds_bytes = 0;            // its launch
    int generation = 0;                          // counts the sets: a captured launch replayed after another set does nothing
    int64_t src_span = 0;                        // bytes of src its images reach
    bool pad = false;                            // mbn_ragged_resizer_create_pad: a letterbox into out_rows x out_cols canvases of `fill`
    uint8_t fill[3] = { 0, 0, 0 };
    void *dev = nullptr, *host = nullptr;        // 64-byte head + mbn_resize_desc [max_batch] (pad: mbn_resize_pad_desc [max_batch])
    hipEvent_t done = nullptr;                   // behind the last upload or launch: the next set waits for it
};

// mbn_ragged_readout_create's handle (mbn_f32_resample.hip): the items of up to max_batch images, on the device and pinned on the host
struct mbn_ragged_readout {
    mbn_context *ctx = nullptr;
    int max_batch = 0;
    int batch = 0;                               // of the last successful set; 0 = none
    int rows = 0, cols = 0, classes = 0;         // its coarse map
    int window = 0, in_rows = 0, in_cols = 0;    // a window set (mbn_ragged_readout_set_window): the network input its rectangles lie in
    mbn_resample_launch_t launch = {};           // its launch: LDS footprint, class chunk, grid.x, the elements of labels / score it reaches
    int generation = 0;                          // counts the sets: a captured launch replayed after another set does nothing
    void *dev = nullptr, *host = nullptr;        // 16-byte head + mbn_label_item or mbn_label_window_item [max_batch] (sized for the latter)
    int64_t *sort = nullptr;                     // [2 * max_batch]: the overlap check's scratch, so that a set allocates nothing
    hipEvent_t done = nullptr;                   // behind the last upload or launch: the next set waits for it
};

// A scratch handle: device memory for the kernels of one family of calls, allocated once for up to max_batch images and `capacity` of the
// family's unit. mbn_scratch_create / _destroy (mbn_abi.hip) serve every family; the public types stay distinct
struct mbn_scratch {
    mbn_context *ctx = nullptr;
    int max_batch = 0;
    int64_t capacity = 0;
    void *scratch = nullptr;
    virtual ~mbn_scratch() = default;            // the context's list deletes a family's handle through this type
};
// mbn_components_create's handle (mbn_i32_components.hip): capacity = max_pixels; scratch = parent [max_pixels], area / rank [max_pixels],
// chunk counts [max_pixels / CHUNK + max_batch], int32
struct mbn_components : mbn_scratch {};
// mbn_panoptic_create's handle (mbn_i32_panoptic.hip): capacity = max_slots; scratch = predicted slots [max_slots][MBN_PANOPTIC_SLOT_WORDS],
// truth slots [max_slots], candidates [max_slots], int32
struct mbn_panoptic : mbn_scratch {};

// the live scratch handles of a context. Its destructor (mbn_abi.hip) frees the stragglers when mbn_shutdown deletes the context
struct mbn_scratch_list {
    std::vector<mbn_scratch *> live;
    ~mbn_scratch_list();
};

struct mbn_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool profiling = false;
    bool ev_valid = false;
    uint32_t literal_quirks = MBN_QUIRKS_KERNEL_CL;
    char last_error[256] = {0};
    char name[128] = {0};
    int num_cus = 256;                           // the PLANNING count every launcher reads: the device's, or fewer (mbn_set_planning_cus)
    int device_cus = 256;                        // compute units of the device itself
    std::vector<hipEvent_t> sync_events;         // mbn_stream_wait: reusable fork/join events (round robin)
    size_t sync_next = 0;
    std::vector<hipEvent_t> pool;                // mbn_profile_begin/end: 2 events per recorded call
    int pool_cap = 0, pool_used = 0;
    bool pool_on = false;
    std::vector<hipEvent_t> marks;               // mbn_mark / mbn_marks_read: step markers (reused across reads)
    size_t marks_used = 0;
    void *lit_ws = nullptr;                      // LITERAL pointwise on v_dot4: packed int8 filter + per-channel weight sums + flag
    size_t lit_ws_bytes = 0;
    std::map<std::pair<uintptr_t, int>, mbn_emul_img> emul_ws;   // pw_emul: pre-split filter images, by (filter pointer, layout) (mbn_f32_pw_x6.hip)
    std::vector<mbn_resizer *> resizers;         // live mbn_resizer_create handles (mbn_shutdown frees the stragglers)
    std::vector<mbn_ragged_resizer *> ragged_resizers;   // live mbn_ragged_resizer_create handles, likewise
    std::vector<mbn_ragged_readout *> ragged_readouts;   // live mbn_ragged_readout_create handles, likewise
    mbn_scratch_list scratches;                  // live mbn_components_create / mbn_panoptic_create handles (freed with the context)
    std::mutex mu;
    std::map<uintptr_t, size_t> allocs;          // buffers handed out by mbn_alloc: base address -> bytes (ordered: mbn_span_check
                                                 // finds the allocation that CONTAINS an interior pointer)
};

static inline int mbn_record_hip_error(mbn_context *ctx, hipError_t e, const char *what)
{
    if (ctx) snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: %s", what, hipGetErrorString(e));
    return MBN_EDEVICE;
}

#define MBN_HIP_TRY(ctx, expr)                                                    \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) return mbn_record_hip_error((ctx), _e, #expr);      \
    } while (0)

// The bounds rule of mbn_alloc (mbn_abi.hip): a pointer inside a tracked buffer must leave room for the bytes the call touches, else MBN_EINVAL
// and last_error names `what`. A null pointer, a span of no bytes and caller-owned memory are not checked.
struct mbn_span { const void *p; double bytes; const char *what; };
int mbn_span_check(mbn_context *ctx, const mbn_span *spans, int n);
// [p, p + p_bytes) and [q, q + q_bytes) share a byte; a null pointer never overlaps
bool mbn_spans_overlap(const void *p, double p_bytes, const void *q, double q_bytes);

// The grid of a persistent kernel: per_cu workgroups on each CU of the planning count, no more than there are units, one at least
static inline unsigned mbn_persistent_grid(int num_cus, int per_cu, long long units)
{
    const long long most = (long long)(num_cus > 0 ? num_cus : 1) * per_cu;
    return (unsigned)(units < most ? (units > 0 ? units : 1) : most);
}

// The scratch handles' life. create: the checks and return codes of mbn_components_create / mbn_panoptic_create (include/mbn.h), `bytes` = the
// family's mbn_*_scratch_bytes answer. destroy: null is MBN_OK; waits for the device (the handle's last launch, whatever the stream).
void mbn_scratch_release(mbn_scratch *h);
int mbn_scratch_destroy(mbn_scratch *h);
template <typename H>
int mbn_scratch_create(mbn_context *ctx, int max_batch, int64_t capacity, int64_t bytes, H **h)
{
    if (!ctx || !h) return MBN_EINVAL;
    *h = nullptr;
    if (max_batch < 1 || capacity < 1) return MBN_EINVAL;
    if (bytes <= 0) return MBN_EUNSUPPORTED;
    H *c = new (std::nothrow) H();
    if (!c) return MBN_ENOMEM;
    c->ctx = ctx;
    c->max_batch = max_batch;
    c->capacity = capacity;
    (void)hipSetDevice(ctx->device);
    if (hipMalloc(&c->scratch, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->scratch = nullptr;
        mbn_scratch_release(c);
        return MBN_ENOMEM;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->scratches.live.push_back(c);
    *h = c;
    return MBN_OK;
}

// Process-wide switches (mbn_tune_set). 0 = shipped default everywhere.
// Two kinds. PRODUCT switches select between code paths that every build contains (the opt-in pw_emul arithmetic, the
// split-K and LITERAL dot4 regimes a test must be able to force, the sub-batch stagger, a forced GEMM tile among the compiled
// ones): relaxed atomics, read once per launch on the host. LAB knobs are A/B hooks of the experiments recorded in
// profiles/LOG.md: they exist only in the lab build (make lab -> libmbn_lab.so, -DMBN_LAB); in the shipped library they are
// compile-time zeros, so every branch on them folds away, the template instantiations only they reach are not compiled,
// and mbn_tune_set answers MBN_EUNSUPPORTED for their keys.
#ifdef MBN_LAB
#define MBN_LAB_KNOB(name) std::atomic<int> name{0}
#define MBN_LAB_BUILD 1
#else
#define MBN_LAB_KNOB(name) static constexpr int name = 0
#define MBN_LAB_BUILD 0
#endif
struct mbn_tunables {
    // ---- product switches
    std::atomic<int> pw_tile{0};      // pointwise GEMM: force a tile shape (0 = per-layer rule); a shape this build does not contain -> MBN_EUNSUPPORTED
    std::atomic<int> lit_dot{0};      // LITERAL pointwise: 0 = v_dot4 path where eligible, 1 = always the scalar kernel
    std::atomic<int> pw_splitk{0};    // fp32 pointwise in the few-tile regime: 0 = split-K kernel (mbn_f32_pw_splitk.hip), 1 = always pw_gemm, 2 = split-K wherever eligible
    std::atomic<int> pw_emul{0};      // fp32 pointwise on the bf16 matrix cores from exact three-way operand splits (mbn_f32_pw_x6.hip): 0 = off, 6 or 9 products
    std::atomic<int> pw_emul_static{0}; // pw_emul: 1 = a filter's image is split once and reused until the filter is rewritten through this library
    std::atomic<int> net_stagger{2};  // layers by which consecutive sub-batch streams are staggered (mbn_net_set_streams)
    std::atomic<int> pw_clock{0};     // 1 = pw_gemm launches accumulate their held core clock (mbn_pw_clock_read)
    std::atomic<int> cu_mask{0};      // streams made by mbn_stream_create alternate between two halves of the chip: 1 = XCDs 0-3 / 4-7, 2 = the two halves of every XCD (round 4 experiment)
    // ---- lab knobs
    MBN_LAB_KNOB(dw_variant);         // depthwise kernel variant
    MBN_LAB_KNOB(dw_nseg);            // force row segments per image (0 = heuristic)
    MBN_LAB_KNOB(pw_stage);           // 1 = register staging instead of direct-to-LDS loads
    MBN_LAB_KNOB(conv_variant);       // conv1 / stem / GEMM-epilogue variants
    MBN_LAB_KNOB(misc);
    MBN_LAB_KNOB(pw_ring);            // bf16 pointwise: 0 = ring kernel for K = 64, 1 = always pw_gemm, 2 = ring wherever eligible
    MBN_LAB_KNOB(pw_xn);              // pointwise GEMM: XCD groups along n (0 = by filter size, 1 = off, 2, 4)
    MBN_LAB_KNOB(dwpw_variant);       // fused block kernel: 0 = shipped choice per shape, 1 = round-1 producer/consumer kernel, 2 = unified-wave kernel,
                                      // 3 = unified with the taps read inside the step, 100 + bits = unified with parts switched off (ablation)
    MBN_LAB_KNOB(exp0);               // scratch knobs of the experiment at hand (kernel files say what they mean where they read them)
    MBN_LAB_KNOB(exp1);
    MBN_LAB_KNOB(exp2);
};
extern mbn_tunables g_mbn_tune;

// Resolved per-call view of (positional args + ext) handed to the kernel launchers.
struct mbn_call {
    mbn_context *ctx;
    hipStream_t stream;
    int batch;
    int act;
    int pad_top, pad_left;
    int in_rows, in_cols;
    int dilation;     // mbn_depthwise: 1 = none (set from ext->dilation by mbn_depthwise; every other call leaves 0)
    int cin;
    int g0, g1;
    uint32_t quirks;
    const float *scale, *shift;
    int dtype;        // MBN_DT_F32, MBN_DT_BF16 or MBN_DT_I8 for the NHWC launchers (storage type of activations)
    int io_flags;     // MBN_IO_IN_F32 / MBN_IO_OUT_F32 (bf16 mode; OUT_F32 also I8), MBN_IO_IN_U8 (convolute)
};

// ---- launchers implemented in the kernel files; each returns MBN_* and launches on c.stream ----
// LITERAL (uint8 planar NCHW / int32) — mbn_literal.hip
int mbn_launch_lit_convolute(const mbn_call &c, uint8_t *out, const uint8_t *r, const uint8_t *g, const uint8_t *b,
                             const int32_t *filt, int rows, int cols, int fs, int stride, int op_size);
int mbn_launch_lit_depthwise(const mbn_call &c, uint8_t *out, const uint8_t *in, const int32_t *filt, int rows,
                             int cols, int fs, int stride, int op_size);
int mbn_launch_lit_pointwise(const mbn_call &c, uint8_t *out, const uint8_t *in, const int32_t *filt, int rows,
                             int cols, int cin, int op_size);
int mbn_launch_lit_pool(const mbn_call &c, uint8_t *out, const uint8_t *in, int rows, int cols, int fs, int op_size);

// NHWC fp32 / bf16 storage (c.dtype), fp32 arithmetic — mbn_f32_dw.hip / mbn_f32_pw.hip / mbn_f32_misc.hip
int mbn_launch_f32_conv(const mbn_call &c, void *out, const void *in, const float *filt, int rows, int cols, int fs,
                        int stride, int op_size);
int mbn_launch_f32_depthwise(const mbn_call &c, void *out, const void *in, const float *filt, int rows, int cols,
                             int fs, int stride, int channels);
int mbn_launch_f32_pointwise(const mbn_call &c, void *out, const void *in, const void *filt, long m, int cin,
                             int op_size);
int mbn_launch_f32_pw_splitk(const mbn_call &c, float *out, const float *in, const float *filt, long m, int cin, int op_size);
int mbn_launch_f32_pw_emul(const mbn_call &c, float *out, const float *in, const float *filt, long m, int cin, int op_size);
int mbn_pw_emul_filter_image(mbn_context *ctx, hipStream_t stream, const float *filt, int n, int k, int bn, int paired,
                             const unsigned **img, unsigned *bytes);
void mbn_pw_emul_invalidate(mbn_context *ctx, const void *dst, size_t bytes);   // caller holds no lock
int mbn_launch_bf16_pw_ring(const mbn_call &c, void *out, const void *in, const void *filt, long m, int cin, int op_size);      // lab build only
int mbn_launch_bf16_pw_wide(const mbn_call &c, void *out, const void *in, const void *fpk, long m, int cin, int op_size);
int mbn_launch_pack_filter_bf16(mbn_context *ctx, hipStream_t s, void *dst, const void *src, int n, int k);
int mbn_bf16_pw_wide_eligible(long m, int cin, int op_size);
int mbn_launch_bf16_pw_rf(const mbn_call &c, void *out, const void *in, const void *filt, long m, int cin, int op_size);          // lab build only (round 6): K = 512, filter in registers
int mbn_launch_bf16_pw_stream(const mbn_call &c, void *out, const void *in, const void *filt, long m, int cin, int op_size, bool m16 = false);
int mbn_launch_bf16_pw_big(const mbn_call &c, void *out, const void *in, const void *filt, long m, int cin, int op_size, long *rows_done);
int mbn_launch_f32_pool(const mbn_call &c, void *out, const void *in, int rows, int cols, int fs, int channels);
// int8 inference mode (MBN_DT_I8: uint8 NHWC activations, int8 filters, mult / bias in c.scale / c.shift) — mbn_i8.hip. The caller has checked
// the shapes (channel counts multiples of 8, K <= 65536) and that every activation / filter pointer is on 8 bytes.
int mbn_launch_i8_conv(const mbn_call &c, uint8_t *out, const void *in, const float *filt, int rows, int cols, int stride, int op_size);
int mbn_launch_i8_depthwise(const mbn_call &c, uint8_t *out, const uint8_t *in, const int8_t *filt, int rows, int cols, int stride, int channels);
int mbn_launch_i8_pointwise(const mbn_call &c, void *out, const uint8_t *in, const int8_t *filt, long m, int cin, int op_size);
int mbn_launch_i8_pool(const mbn_call &c, uint8_t *out, const uint8_t *in, int rows, int cols, int fs, int channels);
size_t mbn_pool_fc_ws_bytes(int channels, int classes);
int mbn_launch_f32_pool_fc(mbn_context *ctx, hipStream_t s, float *out, const float *in, const float *w, const float *bias, void *ws,
                           int batch, int pix, int channels, int classes, int k, float *probs, int32_t *topk_idx, float *topk_prob);
// floor(v / d) == umulhi(v, *m) >> *s for every v < 2^31 (d >= 2); d == 1 gives *m = 0 (callers skip the multiply)
static inline void mbn_udiv_magic(unsigned d, unsigned *m, unsigned *s)
{
    if (d <= 1) { *m = 0; *s = 0; return; }
    unsigned l = 0;
    while ((1u << l) < d) l++;                           // l = ceil(log2 d) >= 1
    const unsigned long long p = 1ull << (31 + l);
    *m = (unsigned)((p + d - 1) / d);                    // ceil(2^(31+l) / d) <= 2^32 - 1 for d >= 2 (== 2^31 for powers of two)
    *s = l - 1;
}

// The fused depthwise -> pointwise block (mbn_dwpw_fused / mbn_dwpw_fused_bf16). Each launcher takes a shape inside
// mbn_block_envelope (the caller has checked it and the pointers) and the block's parameters as the C-ABI's mbn_block_params;
// an fp32 block carries its fp32 pointwise filter in wp_bf16. dwpw2_x6 is the opt-in form on the bf16 matrix cores (pw_emul = 6 | 9):
// MBN_EUNSUPPORTED outside its own limits.
int mbn_launch_f32_dwpw(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
int mbn_launch_f32_dwpw2(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
int mbn_launch_f32_dwpw2_x6(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
int mbn_launch_bf16_dwpw(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
int mbn_launch_bf16_dwpw2(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
// The kernel-argument fields every block form shares (the structs differ, the names agree): the shape, the activations, the depthwise
// parameters and the pointwise scale / shift. esize = bytes per activation element. The pointwise filter is the caller's (wp, or dwpw2_x6's image).
// (the reciprocals of the full-rate window offsets, in the forms that carry them)
template <typename Args>
static inline auto mbn_block_args_inv(Args &a, const mbn_block_shape &s, int) -> decltype((void)a.inv_wo)
{
    a.inv_wo = 1.0f / (float)s.out_cols;
    a.inv_ho = 1.0f / (float)s.out_rows;
}
template <typename Args>
static inline void mbn_block_args_inv(Args &, const mbn_block_shape &, long) {}
template <typename Args>
static inline void mbn_block_args(Args &a, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p, double esize)
{
    a.out = (decltype(a.out))out; a.in = (decltype(a.in))in;
    a.wd = (const float *)p.wd; a.s2 = (const float *)p.s2; a.b2 = (const float *)p.b2; a.s3 = (const float *)p.s3; a.b3 = (const float *)p.b3;
    a.m = (long)s.batch * s.out_rows * s.out_cols;
    a.h = s.in_rows; a.w = s.in_cols; a.ho = s.out_rows; a.wo = s.out_cols;
    a.cin = s.cin; a.cout = s.cout; a.pad_top = s.pad_top; a.pad_left = s.pad_left;
    mbn_udiv_magic((unsigned)s.out_cols, &a.wo_m, &a.wo_s);
    mbn_udiv_magic((unsigned)s.out_rows, &a.ho_m, &a.ho_s);
    a.in_bytes = (unsigned)(esize * s.batch * s.in_rows * s.in_cols * s.cin);
    mbn_block_args_inv(a, s, 0);
}
// short-K pointwise GEMM with the filter slice resident in LDS (mbn_f32_pw3.hip, round 6). Taken where it measured faster than pw_gemm (profiles/r06/l_*:
// layers 5 / 7 / 9 / 11 at batch 256: -22 / -12 / -12 / -7 %, batch 64: -17 / -8 / -9 / -2 %, batch 16: equal; layer 13 (N = 512, four slices): +2 ... +40 %):
// Cin <= 256, Cout <= 256, at least 128 pixels per CU. Same bits as pw_gemm, so the rule may depend on M.
#define MBN_PW3_DEFAULT(m, cin, n, cus) ((cin) <= 256 && (n) <= 256 && (m) >= 128L * (cus))
int mbn_launch_f32_pw3(const mbn_call &c, float *out, const float *in, const float *filt, long m, int cin, int op_size);
// round 6: a run of equal bf16 blocks with the activations resident in LDS (mbn_bf16_res.hip), and the last two blocks + the pool in one launch
// (mbn_bf16_tail.hip). Both take a shape inside their envelope (mbn_envelope.h) and pointers the caller has checked.
int mbn_launch_bf16_tail(mbn_context *ctx, hipStream_t stream, void *out, const void *in, const mbn_block_params *blocks, int batch, int rows, int cols);
int mbn_launch_bf16_res_blocks(mbn_context *ctx, hipStream_t stream, void *out, const void *in, const mbn_block_params *blocks, int nblocks, int batch,
                               int rows, int cols);
// wave-private form of the fp32 block (mbn_f32_dwpw3.hip, round 6): the default for stride-1 blocks with Cin >= 128 (blocks 6-7 and 10-11 of the
// 1.0x network: -9...-12 % and -4...-6 % against dwpw2 in alternating runs, profiles/r06/f_*; equal on 8-9, 8 % slower on 4-5: those stay on dwpw2)
#define MBN_DWPW3_DEFAULT(stride, cin) ((stride) == 1 && (cin) >= 128)
int mbn_f32_dwpw3_eligible(const mbn_context *ctx, const mbn_block_shape &s);      // inside mbn_block_envelope: the form's own limits
int mbn_launch_f32_dwpw3(mbn_context *ctx, hipStream_t stream, const mbn_block_shape &s, void *out, const void *in, const mbn_block_params &p);
// the fused stem: the shape is inside mbn_stem_envelope_hw and the pointers are checked by the caller
int mbn_launch_f32_stem(mbn_context *ctx, hipStream_t stream, float *out, const float *in, const float *w1,
                        const float *s1, const float *b1, const float *wd, const float *s2, const float *b2,
                        const float *wp, const float *s3, const float *b3, int batch, int rows, int cols, int c1, int c3, int in_u8, int bf16);
int mbn_launch_convert(mbn_context *ctx, hipStream_t s, void *dst, const void *src, size_t count, int to_bf16);
int mbn_launch_f32_softmax(mbn_context *ctx, hipStream_t s, float *probs, int32_t *argmax, const float *logits,
                           int batch, int classes);
int mbn_launch_f32_softmax_topk(mbn_context *ctx, hipStream_t s, float *probs, int32_t *topk_idx, float *topk_prob,
                                const float *logits, int batch, int classes, int k);
// dense head read-out (mbn_f32_dense.hip): bilinear upsample by `factor` + argmax over the classes; the shape is inside mbn_upsample_argmax_envelope
int mbn_launch_f32_upsample_argmax(mbn_context *ctx, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows,
                                   int cols, int classes, int factor);
// dense head read-out at any output size (mbn_f32_resample.hip): bilinear resample to out_rows x out_cols + argmax; the shape is inside
// mbn_resample_argmax_envelope, or with rect = (x, y, iw, ih) of the in_rows x in_cols network input (null: the whole map) inside
// mbn_resample_window_envelope. Ragged form: build allocates, plan checks a batch of mbn_label_item, or with `window` of mbn_label_window_item (a
// refused one changes nothing), and enqueues the items' upload.
// q = null: the argmax kernels. q given: the softmax kernels (mbn_resample_softmax_*), which also write prob (may be null when min_prob > 0) and
// store ignore_label where prob < min_prob.
struct mbn_readout_prob { float *prob; float min_prob; int ignore_label; };
int mbn_launch_f32_resample_argmax(mbn_context *ctx, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                   int classes, int in_rows, int in_cols, const int32_t *rect, int out_rows, int out_cols, const mbn_readout_prob *q);
int mbn_ragged_readout_build(mbn_context *ctx, int max_batch, mbn_ragged_readout **r);
void mbn_ragged_readout_release(mbn_ragged_readout *r);
int mbn_ragged_readout_plan(mbn_ragged_readout *r, hipStream_t s, int rows, int cols, int classes, int window, int in_rows, int in_cols,
                            const void *items, int batch);
int mbn_launch_f32_resample_argmax_ragged(mbn_ragged_readout *r, hipStream_t s, int32_t *labels, float *score, const float *logits,
                                          const mbn_readout_prob *q);
// the ensemble read-out of n_views views (logits [n_views][batch][rows][cols][classes]) inside mbn_resample_ensemble_envelope; q as above
int mbn_launch_f32_resample_ensemble(mbn_context *ctx, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                     int classes, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols,
                                     const mbn_readout_prob *q);
// the sliding-window read-out of a grid of tiles (logits [batch][ny * nx][rows][cols][classes]) inside mbn_resample_slide_envelope; q as above
int mbn_launch_f32_resample_slide(mbn_context *ctx, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                  int classes, const mbn_slide *plan, int out_rows, int out_cols, const mbn_readout_prob *q);
// the top-k read-out (mbn_resample_topk_*): labels / score / q->prob are rank-major, rank j at j * plane elements (uniform: plane = batch * out_rows
// * out_cols; ragged: plane_stride). The shape is inside mbn_resample_topk_envelope / mbn_resample_topk_ragged_check; q = null: the logit form
int mbn_launch_f32_resample_topk(mbn_context *ctx, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                 int classes, int in_rows, int in_cols, const int32_t *rect, int out_rows, int out_cols, int k,
                                 const mbn_readout_prob *q);
int mbn_launch_f32_resample_topk_ragged(mbn_ragged_readout *r, hipStream_t s, int32_t *labels, float *score, const float *logits, int k,
                                        int64_t plane_stride, const mbn_readout_prob *q);
// the NLL / Brier read-out (mbn_resample_nll_*): table [temps][classes + 1][4] uint64 +=, nll / brier (either may be null) temperature-major,
// temperature j at j * plane elements (uniform: plane = batch * out_rows * out_cols; ragged: plane_stride); truth at the maps' element offsets.
// The shape is inside mbn_resample_nll_envelope / mbn_resample_nll_ragged_check and inv_temps (host) inside mbn_nll_temps_check
int mbn_launch_f32_resample_nll(mbn_context *ctx, hipStream_t s, void *table, float *nll, float *brier, const float *logits, const void *truth,
                                int truth_bytes, int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t *rect,
                                int out_rows, int out_cols, const float *inv_temps, int temps);
int mbn_launch_f32_resample_nll_ragged(mbn_ragged_readout *r, hipStream_t s, void *table, float *nll, float *brier, int64_t plane_stride,
                                       const float *logits, const void *truth, int truth_bytes, const float *inv_temps, int temps);
// rank score (mbn_i32_topk_rank.hip): ranks [classes + 1][k + 1] uint64 += per truth row the rank at which the truth is among the k label planes
// (plane j at j * plane_stride elements). The arguments are inside mbn_topk_rank_envelope and the pointers checked
int mbn_launch_i32_topk_rank(mbn_context *ctx, hipStream_t s, void *ranks, const void *labels, int k, int64_t plane_stride, const void *truth,
                             int truth_bytes, int classes, int64_t count);
int mbn_launch_i32_topk_rank_ragged(mbn_ragged_readout *r, hipStream_t s, void *ranks, const void *labels, int k, int64_t plane_stride,
                                    const void *truth, int truth_bytes, int classes);
// calibration score (mbn_f32_calibration.hip): calib [bins + 1][4] uint64 += per probability bin the pixels answered, answered correctly, their
// probabilities in 2^-24 fixed point and the pixels abstained; row `bins` the void pixels. The arguments are inside mbn_calibration_envelope and
// the pointers checked; the ragged form scores the items of the handle's set
int mbn_launch_f32_calibration(mbn_context *ctx, hipStream_t s, void *calib, const void *labels, const void *prob, const void *truth, int truth_bytes,
                               int classes, int bins, int64_t count);
int mbn_launch_f32_calibration_ragged(mbn_ragged_readout *r, hipStream_t s, void *calib, const void *labels, const void *prob, const void *truth,
                                      int truth_bytes, int classes, int bins);
// score a segmentation (mbn_i32_confusion.hip): counts [classes + 1][classes + 1] uint64 += the confusion matrix of `count` labels against truth
// (uint8 or int32). The arguments are inside mbn_confusion_envelope and the pointers checked; the ragged form scores the items of the handle's set
int mbn_launch_i32_confusion(mbn_context *ctx, hipStream_t s, void *counts, const void *labels, const void *truth, int truth_bytes, int classes,
                             int64_t count);
int mbn_launch_i32_confusion_ragged(mbn_ragged_readout *r, hipStream_t s, void *counts, const void *labels, const void *truth, int truth_bytes,
                                    int classes);
// resize front-end (mbn_u8_resize.hip): the geometry is inside mbn_resize_envelope; build uploads the tables (blocking), release frees them.
// mirror: the outputs' columns in reverse order (a view's inner image). build_view: the rectangle given (view and fill are non-null)
int mbn_resizer_build(mbn_context *ctx, int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, bool mirror, mbn_resizer **r);
int mbn_resizer_build_pad(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const uint8_t fill[3], mbn_resizer **r);
int mbn_resizer_build_view(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view, const uint8_t fill[3],
                           mbn_resizer **r);
void mbn_resizer_release(mbn_resizer *r);
int mbn_launch_u8_resize(const mbn_resizer *r, hipStream_t s, uint8_t *out, const uint8_t *in, int batch);
// ragged resize (mbn_u8_resize_ragged.hip): build allocates, plan checks and plans a batch and enqueues the descriptors' upload (waits for the handle's
// earlier work first), the launch is asynchronous; taps: the kernel's tap function for one axis into device tables
int mbn_ragged_resizer_build(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, const uint8_t *fill, mbn_ragged_resizer **r);
void mbn_ragged_resizer_release(mbn_ragged_resizer *r);
int mbn_ragged_resizer_plan(mbn_ragged_resizer *r, hipStream_t s, const mbn_resize_item *items, int batch);
int mbn_launch_u8_resize_ragged(mbn_ragged_resizer *r, hipStream_t s, uint8_t *out, const uint8_t *src);
int mbn_launch_resize_taps(hipStream_t s, int filter, int in_size, float b0, float b1, int out_size, int ksize, int32_t *first, int32_t *count, int32_t *weights);
int mbn_launch_normalize(mbn_context *ctx, hipStream_t s, float *out, const uint8_t *in, size_t count, float scale,
                         float bias);

static inline int mbn_same_pad(int in, int out, int k, int stride)
{
    int total = (out - 1) * stride + k - in;
    if (total < 0) total = 0;
    return total / 2;
}
