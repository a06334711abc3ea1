// mbn_abi.hip — the C-ABI of include/mbn.h: context lifecycle, buffers, and the four layer entry points
// that replace the reference's clSetKernelArg + clEnqueueNDRangeKernel protocol
// (MobileNet.c:272-292 convolute, :363-382 depthwise, :453-470 pointwise, :2640-2656 pool).
//
// No CPU fallback exists: without a HIP device mbn_init returns MBN_ENODEVICE and nothing computes.
#include "mbn_internal.h"

#include <initializer_list>
#include <new>

mbn_tunables g_mbn_tune;

// Buffer-size guard. Every buffer handed out by mbn_alloc is recorded with its size; when a pointer given to a call
// lies inside one of them, the bytes the call is about to touch must fit in what is left of that allocation, otherwise
// the call is a caller error (MBN_EINVAL) instead of a GPU memory fault. Caller-owned memory (hipMalloc, a torch tensor)
// is not in the map and is not checked. Cause on record (round 1, gpurun_out/fault.log): the C host uploaded a uint8
// image (3*96*96*3 bytes) and issued the fp32 first-layer kernel on it, which read 4x the buffer.
int mbn_span_check(mbn_context *ctx, const mbn_span *sp, int n)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->allocs.empty()) return MBN_OK;
    for (int i = 0; i < n; i++) {
        if (!sp[i].p || sp[i].bytes <= 0) continue;
        const uintptr_t a = (uintptr_t)sp[i].p;
        auto it = ctx->allocs.upper_bound(a);
        if (it == ctx->allocs.begin()) continue;
        --it;
        if (a >= it->first + it->second) continue;                 // not inside any of our buffers
        const double room = (double)(it->first + it->second - a);
        if (sp[i].bytes > room) {
            snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: call touches %.0f bytes, %.0f left in its %zu-byte mbn_alloc buffer",
                     sp[i].what, sp[i].bytes, room, it->second);
            return MBN_EINVAL;
        }
    }
    return MBN_OK;
}

bool mbn_spans_overlap(const void *p, double p_bytes, const void *q, double q_bytes)
{
    if (!p || !q) return false;
    const double x = (double)(uintptr_t)p, y = (double)(uintptr_t)q;
    return x < y + q_bytes && y < x + p_bytes;
}

void mbn_scratch_release(mbn_scratch *h)
{
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
}

mbn_scratch_list::~mbn_scratch_list()
{
    for (mbn_scratch *h : live) mbn_scratch_release(h);
}

int mbn_scratch_destroy(mbn_scratch *h)
{
    if (!h) return MBN_OK;
    mbn_context *ctx = h->ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto &live = ctx->scratches.live;
        for (auto it = live.begin(); it != live.end(); ++it)
            if (*it == h) { live.erase(it); break; }
    }
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipDeviceSynchronize());                    // its last launch, whatever the stream
    mbn_scratch_release(h);
    return MBN_OK;
}

namespace {

#define MBN_SPANS(ctx, ...)                                                               \
    do {                                                                                  \
        const mbn_span _sp[] = { __VA_ARGS__ };                                           \
        const int _rc = mbn_span_check((ctx), _sp, (int)(sizeof(_sp) / sizeof(_sp[0])));  \
        if (_rc != MBN_OK) return _rc;                                                    \
    } while (0)

// Pointers of a fused launch: MBN_EINVAL when one is null, else MBN_EUNSUPPORTED when one is not on 16 bytes (the fused kernels
// load and store with 16-byte accesses), else MBN_OK
int check_ptrs(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (!p) return MBN_EINVAL;
    for (const void *p : ptrs)
        if ((uintptr_t)p % 16) return MBN_EUNSUPPORTED;
    return MBN_OK;
}
int check_ptrs(const mbn_block_params &b) { return check_ptrs({ b.wd, b.s2, b.b2, b.wp_bf16, b.s3, b.b3 }); }

// element size of an activation tensor of the call: bf16 mode stores 2 bytes unless the io flag says fp32
inline double esz_in(const mbn_call &c) { return c.dtype == MBN_DT_BF16 && !(c.io_flags & MBN_IO_IN_F32) ? 2.0 : 4.0; }
inline double esz_out(const mbn_call &c) { return c.dtype == MBN_DT_BF16 && !(c.io_flags & MBN_IO_OUT_F32) ? 2.0 : 4.0; }

// Library-owned images derived from [lo, hi) (the pre-split filter images of pw_emul): taken out of the map under the lock,
// released by the caller once the device is idle (they may be in use on any of the net runner's sub-batch streams).
std::vector<void *> take_derived(mbn_context *ctx, uintptr_t lo, uintptr_t hi)
{
    std::vector<void *> gone;
    for (auto it = ctx->emul_ws.begin(); it != ctx->emul_ws.end();) {
        if (it->first.first < hi && it->first.first + it->second.src_bytes > lo) {
            gone.push_back(it->second.p);
            it = ctx->emul_ws.erase(it);
        } else ++it;
    }
    return gone;
}

}   // namespace

extern "C" {

static std::atomic<int> *tune_slot(const char *key, bool *lab_only)
{
    *lab_only = false;
    if (!key) return nullptr;
    if (!strcmp(key, "pw_tile")) return &g_mbn_tune.pw_tile;
    if (!strcmp(key, "net_stagger")) return &g_mbn_tune.net_stagger;
    if (!strcmp(key, "pw_splitk")) return &g_mbn_tune.pw_splitk;
    if (!strcmp(key, "pw_emul")) return &g_mbn_tune.pw_emul;
    if (!strcmp(key, "pw_emul_static")) return &g_mbn_tune.pw_emul_static;
    if (!strcmp(key, "lit_dot")) return &g_mbn_tune.lit_dot;
    if (!strcmp(key, "pw_clock")) return &g_mbn_tune.pw_clock;
    static const char *const lab_keys[] = { "dw_variant", "dw_nseg", "pw_stage", "conv_variant", "misc", "pw_ring", "pw_xn", "dwpw_variant",
                                            "exp0", "exp1", "exp2", "cu_mask" };
    for (const char *k : lab_keys)
        if (!strcmp(key, k)) *lab_only = true;
#ifdef MBN_LAB
    if (!strcmp(key, "dw_variant")) return &g_mbn_tune.dw_variant;
    if (!strcmp(key, "dw_nseg")) return &g_mbn_tune.dw_nseg;
    if (!strcmp(key, "pw_stage")) return &g_mbn_tune.pw_stage;
    if (!strcmp(key, "conv_variant")) return &g_mbn_tune.conv_variant;
    if (!strcmp(key, "misc")) return &g_mbn_tune.misc;
    if (!strcmp(key, "pw_ring")) return &g_mbn_tune.pw_ring;
    if (!strcmp(key, "pw_xn")) return &g_mbn_tune.pw_xn;
    if (!strcmp(key, "dwpw_variant")) return &g_mbn_tune.dwpw_variant;
    if (!strcmp(key, "exp0")) return &g_mbn_tune.exp0;
    if (!strcmp(key, "exp1")) return &g_mbn_tune.exp1;
    if (!strcmp(key, "exp2")) return &g_mbn_tune.exp2;
    if (!strcmp(key, "cu_mask")) return &g_mbn_tune.cu_mask;
#endif
    return nullptr;
}

int mbn_lab_build(void) { return MBN_LAB_BUILD; }

int mbn_tune_set(const char *key, int value)
{
    bool lab_only;
    std::atomic<int> *p = tune_slot(key, &lab_only);
    if (!p) return lab_only ? MBN_EUNSUPPORTED : MBN_ENOTFOUND;      // a lab knob in the shipped library
    p->store(value, std::memory_order_relaxed);
    return MBN_OK;
}

int mbn_tune_get(const char *key, int *value)
{
    bool lab_only;
    std::atomic<int> *p = tune_slot(key, &lab_only);
    if (!value) return MBN_EINVAL;
    if (!p) {
        if (!lab_only) return MBN_ENOTFOUND;
        *value = 0;                                                   // what the shipped library behaves like
        return MBN_OK;
    }
    *value = p->load(std::memory_order_relaxed);
    return MBN_OK;
}

int mbn_device_count(int *count)
{
    if (!count) return MBN_EINVAL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return MBN_OK;
}

int mbn_init(int device_ordinal, mbn_context **out)
{
    if (!out) return MBN_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MBN_ENODEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return MBN_ENODEVICE;
    mbn_context *ctx = new (std::nothrow) mbn_context();
    if (!ctx) return MBN_ENOMEM;
    ctx->device = device_ordinal;
    hipError_t e = hipSetDevice(device_ordinal);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_start);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_stop);
    if (e != hipSuccess) {
        if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return MBN_EDEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) {
        snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
        ctx->num_cus = ctx->device_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    *out = ctx;
    return MBN_OK;
}

int mbn_shutdown(mbn_context *ctx)
{
    if (!ctx) return MBN_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &kv : ctx->allocs) (void)hipFree((void *)kv.first);
    if (ctx->lit_ws) (void)hipFree(ctx->lit_ws);
    for (auto &kv : ctx->emul_ws) (void)hipFree(kv.second.p);
    for (mbn_resizer *r : ctx->resizers) mbn_resizer_release(r);
    for (mbn_ragged_resizer *r : ctx->ragged_resizers) mbn_ragged_resizer_release(r);
    for (mbn_ragged_readout *r : ctx->ragged_readouts) mbn_ragged_readout_release(r);
    ctx->allocs.clear();
    for (hipEvent_t e : ctx->pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->marks) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->sync_events) (void)hipEventDestroy(e);
    (void)hipEventDestroy(ctx->ev_start);
    (void)hipEventDestroy(ctx->ev_stop);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MBN_OK;
}

int mbn_device_name(mbn_context *ctx, char *buf, size_t buflen)
{
    if (!ctx || !buf || buflen == 0) return MBN_EINVAL;
    snprintf(buf, buflen, "%s", ctx->name);
    return MBN_OK;
}

int mbn_device_pci_bus_id(mbn_context *ctx, char *buf, size_t buflen)
{
    if (!ctx || !buf || buflen < 16) return MBN_EINVAL;
    buf[0] = 0;
    MBN_HIP_TRY(ctx, hipDeviceGetPCIBusId(buf, (int)buflen, ctx->device));
    return MBN_OK;
}

int mbn_device_cus(mbn_context *ctx, int *count)
{
    if (!ctx || !count) return MBN_EINVAL;
    *count = ctx->num_cus;
    return MBN_OK;
}

int mbn_set_planning_cus(mbn_context *ctx, int cus)
{
    if (!ctx || cus < 0 || cus > ctx->device_cus) return MBN_EINVAL;
    ctx->num_cus = cus ? cus : ctx->device_cus;
    return MBN_OK;
}

const char *mbn_last_device_error(mbn_context *ctx) { return ctx ? ctx->last_error : "no context"; }

int mbn_set_literal_quirks(mbn_context *ctx, uint32_t quirks)
{
    if (!ctx || (quirks & ~MBN_QUIRKS_KERNEL_CL)) return MBN_EINVAL;
    ctx->literal_quirks = quirks;
    return MBN_OK;
}

int mbn_get_stream(mbn_context *ctx, void **stream)
{
    if (!ctx || !stream) return MBN_EINVAL;
    *stream = (void *)ctx->stream;
    return MBN_OK;
}

int mbn_stream_create(mbn_context *ctx, void **stream)
{
    if (!ctx || !stream) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s;
    const int cm = g_mbn_tune.cu_mask;
    if (cm == 1 || cm == 2) {
        // LAB experiment (round 4, profiles/r04/j_streams_cu_mask.txt: XCD halves equal to the shared chip within 0.2 %, halves of every XCD -2.3 %): sub-batch streams confined to disjoint halves of the chip, so that one stream's HBM-bound kernels run beside the
        // other's MFMA-bound ones instead of time-slicing the same CUs. CU-mask bit i is CU i / 8 of XCD i % 8 (the driver deals the bits round the XCDs)
        static std::atomic<int> seq{0};
        const int half = seq.fetch_add(1) & 1;
        uint32_t mask[8];
        for (int w = 0; w < 8; w++) {
            uint32_t m = 0;
            for (int b = 0; b < 32; b++) {
                const int i = 32 * w + b;
                const bool mine = cm == 1 ? ((i & 7) < 4) == (half == 0) : (i < 128) == (half == 0);
                if (mine) m |= 1u << b;
            }
            mask[w] = m;
        }
        MBN_HIP_TRY(ctx, hipExtStreamCreateWithCUMask(&s, 8, mask));
        *stream = (void *)s;
        return MBN_OK;
    }
    MBN_HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return MBN_OK;
}

int mbn_stream_destroy(mbn_context *ctx, void *stream)
{
    if (!ctx || !stream) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    MBN_HIP_TRY(ctx, hipStreamDestroy((hipStream_t)stream));
    return MBN_OK;
}

int mbn_stream_wait(mbn_context *ctx, void *waiter, void *signaler)
{
    if (!ctx) return MBN_EINVAL;
    hipStream_t w = waiter ? (hipStream_t)waiter : ctx->stream, sg = signaler ? (hipStream_t)signaler : ctx->stream;
    if (w == sg) return MBN_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->sync_events.size() < 64) {
        hipEvent_t e;
        MBN_HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->sync_events.push_back(e);
        ctx->sync_next = ctx->sync_events.size() - 1;
    } else ctx->sync_next = (ctx->sync_next + 1) % ctx->sync_events.size();
    hipEvent_t e = ctx->sync_events[ctx->sync_next];      // re-recording an event is legal: earlier waits keep their capture
    MBN_HIP_TRY(ctx, hipEventRecord(e, sg));
    MBN_HIP_TRY(ctx, hipStreamWaitEvent(w, e, 0));
    return MBN_OK;
}

int mbn_graph_begin(mbn_context *ctx, void *stream)
{
    if (!ctx) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_HIP_TRY(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    return MBN_OK;
}

int mbn_graph_end(mbn_context *ctx, void *stream, void **graph_exec)
{
    if (!ctx || !graph_exec) return MBN_EINVAL;
    *graph_exec = nullptr;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    hipGraph_t g = nullptr;
    MBN_HIP_TRY(ctx, hipStreamEndCapture(s, &g));
    hipGraphExec_t ge = nullptr;
    hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return mbn_record_hip_error(ctx, e, "hipGraphInstantiate");
    *graph_exec = (void *)ge;
    return MBN_OK;
}

int mbn_graph_launch(mbn_context *ctx, void *graph_exec, void *stream)
{
    if (!ctx || !graph_exec) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipGraphLaunch((hipGraphExec_t)graph_exec, stream ? (hipStream_t)stream : ctx->stream));
    return MBN_OK;
}

int mbn_graph_destroy(mbn_context *ctx, void *graph_exec)
{
    if (!ctx) return MBN_EINVAL;
    if (!graph_exec) return MBN_OK;
    MBN_HIP_TRY(ctx, hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return MBN_OK;
}

int mbn_alloc(mbn_context *ctx, size_t bytes, void **dptr)
{
    if (!ctx || !dptr || bytes == 0) return MBN_EINVAL;
    *dptr = nullptr;
    (void)hipSetDevice(ctx->device);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) return MBN_ENOMEM;
    if (e != hipSuccess) return mbn_record_hip_error(ctx, e, "hipMalloc");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->allocs[(uintptr_t)p] = bytes;
    *dptr = p;
    return MBN_OK;
}

int mbn_free(mbn_context *ctx, void *dptr)
{
    if (!ctx) return MBN_EINVAL;
    if (!dptr) return MBN_OK;
    std::vector<void *> gone;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->allocs.find((uintptr_t)dptr);
        if (it == ctx->allocs.end()) return MBN_EINVAL;   // not ours: caller-owned memory is never freed here
        const size_t freed = it->second;
        ctx->allocs.erase(it);
        gone = take_derived(ctx, (uintptr_t)dptr, (uintptr_t)dptr + freed);     // images of filters inside the freed buffer (they leaked)
    }
    (void)hipSetDevice(ctx->device);
    if (!gone.empty()) MBN_HIP_TRY(ctx, hipDeviceSynchronize());
    else MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (void *p : gone) (void)hipFree(p);
    MBN_HIP_TRY(ctx, hipFree(dptr));
    return MBN_OK;
}

int mbn_forget(mbn_context *ctx, const void *dptr, size_t bytes)
{
    if (!ctx) return MBN_EINVAL;
    if (!dptr || bytes == 0) return MBN_OK;
    std::vector<void *> gone;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        gone = take_derived(ctx, (uintptr_t)dptr, (uintptr_t)dptr + bytes);
    }
    if (gone.empty()) return MBN_OK;
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipDeviceSynchronize());
    for (void *p : gone) (void)hipFree(p);
    return MBN_OK;
}

int mbn_upload(mbn_context *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx || !dst || !src) return MBN_EINVAL;
    if (bytes == 0) return MBN_OK;
    MBN_SPANS(ctx, { dst, (double)bytes, "upload destination" });
    mbn_pw_emul_invalidate(ctx, dst, bytes);
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // blocking like CL_TRUE, MobileNet.c:350
    return MBN_OK;
}

int mbn_download(mbn_context *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx || !dst || !src) return MBN_EINVAL;
    if (bytes == 0) return MBN_OK;
    MBN_SPANS(ctx, { src, (double)bytes, "download source" });
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // blocking like CL_TRUE, MobileNet.c:395
    return MBN_OK;
}

int mbn_memset(mbn_context *ctx, void *dst, int byte, size_t bytes)
{
    if (!ctx || !dst) return MBN_EINVAL;
    if (bytes == 0) return MBN_OK;
    MBN_SPANS(ctx, { dst, (double)bytes, "memset destination" });
    mbn_pw_emul_invalidate(ctx, dst, bytes);
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipMemsetAsync(dst, byte, bytes, ctx->stream));
    return MBN_OK;
}

int mbn_sync(mbn_context *ctx)
{
    if (!ctx) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MBN_OK;
}

int mbn_set_profiling(mbn_context *ctx, int enabled)
{
    if (!ctx) return MBN_EINVAL;
    ctx->profiling = enabled != 0;
    ctx->ev_valid = false;
    return MBN_OK;
}

int mbn_last_kernel_ms(mbn_context *ctx, float *ms)
{
    if (!ctx || !ms) return MBN_EINVAL;
    if (!ctx->ev_valid) return MBN_EINVAL;
    MBN_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    MBN_HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev_start, ctx->ev_stop));
    return MBN_OK;
}

int mbn_profile_begin(mbn_context *ctx, int capacity)
{
    if (!ctx || capacity <= 0 || capacity > (1 << 20)) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    while ((int)ctx->pool.size() < 2 * capacity) {
        hipEvent_t e;
        MBN_HIP_TRY(ctx, hipEventCreate(&e));
        ctx->pool.push_back(e);
    }
    ctx->pool_cap = capacity;
    ctx->pool_used = 0;
    ctx->pool_on = true;
    return MBN_OK;
}

int mbn_profile_pause(mbn_context *ctx, int paused)
{
    if (!ctx) return MBN_EINVAL;
    ctx->pool_on = !paused && ctx->pool_cap > 0;
    return MBN_OK;
}

int mbn_profile_end(mbn_context *ctx, float *ms, int ms_capacity, int *count)
{
    if (!ctx || !ms || !count || ms_capacity < 0) return MBN_EINVAL;
    ctx->pool_on = false;
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipDeviceSynchronize());
    int n = ctx->pool_used < ms_capacity ? ctx->pool_used : ms_capacity;
    for (int i = 0; i < n; i++) MBN_HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->pool[2 * i], ctx->pool[2 * i + 1]));
    *count = n;
    return MBN_OK;
}

int mbn_mark(mbn_context *ctx, void *stream)
{
    if (!ctx) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->marks_used == ctx->marks.size()) {
        if (ctx->marks.size() >= (1u << 20)) return MBN_ENOMEM;
        hipEvent_t e;
        MBN_HIP_TRY(ctx, hipEventCreate(&e));
        ctx->marks.push_back(e);
    }
    MBN_HIP_TRY(ctx, hipEventRecord(ctx->marks[ctx->marks_used], stream ? (hipStream_t)stream : ctx->stream));
    ctx->marks_used++;
    return MBN_OK;
}

int mbn_marks_read(mbn_context *ctx, float *ms_between, int capacity, int *count)
{
    if (!ctx || !count || capacity < 0 || (capacity > 0 && !ms_between)) return MBN_EINVAL;
    (void)hipSetDevice(ctx->device);
    const size_t used = ctx->marks_used;
    ctx->marks_used = 0;
    *count = 0;
    if (used == 0) return MBN_OK;
    MBN_HIP_TRY(ctx, hipEventSynchronize(ctx->marks[used - 1]));
    int n = 0;
    for (size_t i = 1; i < used && n < capacity; i++, n++)
        MBN_HIP_TRY(ctx, hipEventElapsedTime(&ms_between[n], ctx->marks[i - 1], ctx->marks[i]));
    *count = n;
    return MBN_OK;
}

}   // extern "C"

// --------------------------------------------------------------------------- call resolution

namespace {


struct Scope {   // hipEvent pair around one layer call when profiling is on (MobileNet.c:301-305 analogue)
    mbn_context *ctx;
    hipStream_t s;
    int slot = -1;
    bool capturing = false;
    Scope(mbn_context *c, hipStream_t st) : ctx(c), s(st)
    {
        (void)hipSetDevice(ctx->device);
        if (ctx->profiling || ctx->pool_on) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        }
        if (capturing) return;
        if (ctx->profiling) (void)hipEventRecord(ctx->ev_start, s);
        if (ctx->pool_on && ctx->pool_used < ctx->pool_cap) {
            slot = ctx->pool_used++;
            (void)hipEventRecord(ctx->pool[2 * slot], s);
        }
    }
    int finish(int rc)
    {
        if (slot >= 0) (void)hipEventRecord(ctx->pool[2 * slot + 1], s);
        if (ctx->profiling && !capturing) {
            (void)hipEventRecord(ctx->ev_stop, s);
            ctx->ev_valid = true;
        }
        if (rc != MBN_OK) return rc;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return mbn_record_hip_error(ctx, e, "kernel launch");
        return MBN_OK;
    }
};

__global__ void mbn_null_kernel() {}

int resolve(mbn_context *ctx, const mbn_layer_ext *ext, mbn_call *c, int *dtype)
{
    if (!ctx) return MBN_EINVAL;
    memset(c, 0, sizeof(*c));
    c->ctx = ctx;
    c->stream = ctx->stream;
    c->batch = 1;
    c->act = MBN_ACT_RELU;
    c->pad_top = c->pad_left = -1;
    c->quirks = ctx->literal_quirks;
    *dtype = MBN_DT_U8;
    if (!ext) return MBN_OK;
    if (ext->struct_size != sizeof(mbn_layer_ext)) return MBN_EINVAL;
    *dtype = ext->dtype;
    if (ext->dtype != MBN_DT_U8 && ext->dtype != MBN_DT_F32 && ext->dtype != MBN_DT_BF16 && ext->dtype != MBN_DT_I8) return MBN_EINVAL;
    if (ext->dtype == MBN_DT_U8 && ext->layout != MBN_LAYOUT_NCHW_PLANAR) return MBN_EUNSUPPORTED;
    if (ext->dtype != MBN_DT_U8 && ext->layout != MBN_LAYOUT_NHWC) return MBN_EUNSUPPORTED;
    if (ext->io_flags & ~(MBN_IO_IN_F32 | MBN_IO_OUT_F32 | MBN_IO_IN_U8 | MBN_IO_FILT_PACKED)) return MBN_EINVAL;
    c->dtype = ext->dtype;
    // IN_F32 / OUT_F32 only mean something in bf16 mode, and OUT_F32 in I8 mode (the FC's logits); IN_U8 (raw image into convolute)
    // applies to fp32, bf16 and I8
    c->io_flags = ext->dtype == MBN_DT_BF16 ? ext->io_flags
                : ext->dtype == MBN_DT_I8   ? (ext->io_flags & (MBN_IO_IN_U8 | MBN_IO_OUT_F32))
                                            : (ext->io_flags & MBN_IO_IN_U8);
    if (ext->batch < 0) return MBN_EINVAL;
    c->batch = ext->batch > 0 ? ext->batch : 1;
    if (ext->act < MBN_ACT_NONE || ext->act > MBN_ACT_RELU6) return MBN_EINVAL;
    c->act = ext->act;
    c->pad_top = ext->pad_top;
    c->pad_left = ext->pad_left;
    c->in_rows = ext->in_rows;
    c->in_cols = ext->in_cols;
    c->cin = ext->cin;
    c->g0 = ext->gsize0;
    c->g1 = ext->gsize1;
    if (ext->quirks_valid) {
        if (ext->quirks & ~MBN_QUIRKS_KERNEL_CL) return MBN_EINVAL;
        c->quirks = ext->quirks;
    }
    c->scale = (const float *)ext->scale;
    c->shift = (const float *)ext->shift;
    if (ext->stream) c->stream = (hipStream_t)ext->stream;
    return MBN_OK;
}

// I8 mode (mbn.h, "int8 inference mode"): the checks every I8 layer call shares. Activations and filters are read and written in 4- to
// 16-byte pieces, so their pointers must be on 8 bytes; channel counts are multiples of 8; mult / bias are required.
int i8_check(const mbn_call &c, std::initializer_list<const void *> ptrs, bool need_params)
{
    if (need_params && (!c.scale || !c.shift)) return MBN_EINVAL;
    if (c.act == MBN_ACT_NONE && !(c.io_flags & MBN_IO_OUT_F32)) return MBN_EINVAL;
    for (const void *p : ptrs)
        if ((uintptr_t)p % 8) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

}   // namespace

extern "C" {

int mbn_profile_null(mbn_context *ctx, int with_kernel, void *stream)
{
    if (!ctx) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    Scope sc(ctx, s);
    if (with_kernel) hipLaunchKernelGGL(mbn_null_kernel, dim3(1), dim3(64), 0, s);
    return sc.finish(MBN_OK);
}

int mbn_convolute(mbn_context *ctx, void *output, const void *inp_r, const void *inp_g, const void *inp_b,
                  const void *filter_k, int rows, int cols, int filtersize, int stride, int op_size,
                  const mbn_layer_ext *ext)
{
    mbn_call c;
    int dtype;
    int rc = resolve(ctx, ext, &c, &dtype);
    if (rc != MBN_OK) return rc;
    if (!output || !inp_r || !filter_k) return MBN_EINVAL;
    if (rows <= 0 || cols <= 0 || op_size <= 0 || stride <= 0 || filtersize <= 0 || !(filtersize & 1))
        return MBN_EINVAL;
    // every argument check comes before the profiling Scope: an MBN_EINVAL must not consume an event slot
    if (dtype == MBN_DT_U8) {
        if (!inp_g || !inp_b) return MBN_EINVAL;
        if (rows / stride <= 0 || cols / stride <= 0) return MBN_EINVAL;
        const double plane = (double)rows * cols, oplane = (c.quirks & MBN_Q_LITERAL_INDEX) ? (double)(rows / 2) * (cols / 2)
                                                                                               : (double)(rows / stride) * (cols / stride);
        MBN_SPANS(ctx, { inp_r, plane * c.batch, "convolute inp_image_r" }, { inp_g, plane * c.batch, "convolute inp_image_g" },
                  { inp_b, plane * c.batch, "convolute inp_image_b" }, { output, oplane * op_size * c.batch, "convolute output" },
                  { filter_k, 4.0 * op_size * 3 * filtersize * filtersize, "convolute filter" });
        Scope sc(ctx, c.stream);
        return sc.finish(mbn_launch_lit_convolute(c, (uint8_t *)output, (const uint8_t *)inp_r, (const uint8_t *)inp_g,
                                                  (const uint8_t *)inp_b, (const int32_t *)filter_k, rows, cols,
                                                  filtersize, stride, op_size));
    }
    if (c.cin <= 0) c.cin = 3;
    if (dtype == MBN_DT_I8) {
        if (filtersize != 3 || stride > 2 || c.cin != 3 || (c.io_flags & MBN_IO_OUT_F32)) return MBN_EUNSUPPORTED;
        if ((rc = i8_check(c, { output }, true)) != MBN_OK) return rc;
        if (op_size % 8) return MBN_EUNSUPPORTED;
        const double orow = (rows + stride - 1) / stride, ocol = (cols + stride - 1) / stride;
        const double in_es = (c.io_flags & MBN_IO_IN_U8) ? 1.0 : 4.0;
        MBN_SPANS(ctx, { inp_r, in_es * c.batch * rows * cols * c.cin, "convolute image" },
                  { output, 1.0 * c.batch * orow * ocol * op_size, "convolute output" },
                  { filter_k, 4.0 * 9 * c.cin * op_size, "convolute filter" },
                  { c.scale, 4.0 * op_size, "convolute mult" }, { c.shift, 4.0 * op_size, "convolute bias" });
        Scope sc(ctx, c.stream);
        return sc.finish(mbn_launch_i8_conv(c, (uint8_t *)output, inp_r, (const float *)filter_k, rows, cols, stride, op_size));
    }
    {
        const double orow = (rows + stride - 1) / stride, ocol = (cols + stride - 1) / stride;
        const double in_es = (c.io_flags & MBN_IO_IN_U8) ? 1.0 : esz_in(c);
        MBN_SPANS(ctx, { inp_r, in_es * c.batch * rows * cols * c.cin, "convolute image" },
                  { output, esz_out(c) * c.batch * orow * ocol * op_size, "convolute output" },
                  { filter_k, 4.0 * filtersize * filtersize * c.cin * op_size, "convolute filter" },
                  { c.scale, 4.0 * op_size, "convolute scale" }, { c.shift, 4.0 * op_size, "convolute shift" });
    }
    Scope sc(ctx, c.stream);
    return sc.finish(mbn_launch_f32_conv(c, output, inp_r, (const float *)filter_k, rows, cols, filtersize, stride, op_size));
}

int mbn_depthwise(mbn_context *ctx, void *output, const void *inp_image, const void *filter_k, int rows, int cols,
                  int filtersize, int stride, int op_size, const mbn_layer_ext *ext)
{
    mbn_call c;
    int dtype;
    int rc = resolve(ctx, ext, &c, &dtype);
    if (rc != MBN_OK) return rc;
    if (!output || !inp_image || !filter_k) return MBN_EINVAL;
    if (rows <= 0 || cols <= 0 || op_size <= 0 || stride <= 0 || filtersize <= 0 || !(filtersize & 1))
        return MBN_EINVAL;
    if (c.in_rows <= 0) c.in_rows = rows * stride;
    if (c.in_cols <= 0) c.in_cols = cols * stride;
    // ext->dilation (read here only): 0 or 1 = none; fp32 and bf16 honour it, LITERAL and I8 have no dilated form
    c.dilation = 1;
    if (ext) {
        if (ext->dilation < 0) return MBN_EINVAL;
        if (ext->dilation > 1) c.dilation = ext->dilation;
    }
    if (c.dilation > 1 && (dtype == MBN_DT_U8 || dtype == MBN_DT_I8)) return MBN_EUNSUPPORTED;
    if (dtype == MBN_DT_I8) {
        if (filtersize != 3 || stride > 2 || (c.io_flags & MBN_IO_OUT_F32)) return MBN_EUNSUPPORTED;
        if ((rc = i8_check(c, { output, inp_image, filter_k }, true)) != MBN_OK) return rc;
        if (op_size % 8) return MBN_EUNSUPPORTED;
        MBN_SPANS(ctx, { inp_image, 1.0 * c.batch * c.in_rows * c.in_cols * op_size, "depthwise input" },
                  { output, 1.0 * c.batch * rows * cols * op_size, "depthwise output" }, { filter_k, 9.0 * op_size, "depthwise filter" },
                  { c.scale, 4.0 * op_size, "depthwise mult" }, { c.shift, 4.0 * op_size, "depthwise bias" });
        Scope sc(ctx, c.stream);
        return sc.finish(mbn_launch_i8_depthwise(c, (uint8_t *)output, (const uint8_t *)inp_image, (const int8_t *)filter_k, rows, cols, stride,
                                                 op_size));
    }
    {
        const double es = dtype == MBN_DT_U8 ? 1.0 : esz_in(c), fes = 4.0 * filtersize * filtersize * op_size;
        MBN_SPANS(ctx, { inp_image, es * c.batch * c.in_rows * c.in_cols * op_size, "depthwise input" },
                  { output, (dtype == MBN_DT_U8 ? 1.0 : esz_out(c)) * c.batch * rows * cols * op_size, "depthwise output" },
                  { filter_k, fes, "depthwise filter" }, { c.scale, 4.0 * op_size, "depthwise scale" },
                  { c.shift, 4.0 * op_size, "depthwise shift" });
    }
    Scope sc(ctx, c.stream);
    if (dtype == MBN_DT_U8)
        return sc.finish(mbn_launch_lit_depthwise(c, (uint8_t *)output, (const uint8_t *)inp_image,
                                                  (const int32_t *)filter_k, rows, cols, filtersize, stride, op_size));
    return sc.finish(mbn_launch_f32_depthwise(c, output, inp_image, (const float *)filter_k, rows, cols, filtersize, stride,
                                              op_size));
}

int mbn_pointwise(mbn_context *ctx, void *output, const void *inp_image, const void *filter_k, int rows, int cols,
                  int filtersize, int op_size, const mbn_layer_ext *ext)
{
    mbn_call c;
    int dtype;
    int rc = resolve(ctx, ext, &c, &dtype);
    if (rc != MBN_OK) return rc;
    if (!output || !inp_image || !filter_k) return MBN_EINVAL;
    if (rows <= 0 || cols <= 0 || op_size <= 0 || filtersize <= 0) return MBN_EINVAL;
    if (dtype == MBN_DT_I8) {
        const bool f32 = (c.io_flags & MBN_IO_OUT_F32) != 0;
        if ((rc = i8_check(c, { output, inp_image, filter_k }, true)) != MBN_OK) return rc;
        if (f32 && c.act != MBN_ACT_NONE) return MBN_EINVAL;                  // fp32 logits are y itself: no activation applies
        if (filtersize % 8 || filtersize > 65536 || (!f32 && op_size % 8)) return MBN_EUNSUPPORTED;   // |acc| < 2^31 needs K <= 65536
        const double px = (double)c.batch * rows * cols;
        MBN_SPANS(ctx, { inp_image, px * filtersize, "pointwise input" }, { output, (f32 ? 4.0 : 1.0) * px * op_size, "pointwise output" },
                  { filter_k, 1.0 * op_size * filtersize, "pointwise filter" },
                  { c.scale, 4.0 * op_size, "pointwise mult" }, { c.shift, 4.0 * op_size, "pointwise bias" });
        Scope sc(ctx, c.stream);
        return sc.finish(mbn_launch_i8_pointwise(c, output, (const uint8_t *)inp_image, (const int8_t *)filter_k, (long)c.batch * rows * cols,
                                                 filtersize, op_size));
    }
    {
        const double px = (double)c.batch * rows * cols, lit = dtype == MBN_DT_U8;
        MBN_SPANS(ctx, { inp_image, (lit ? 1.0 : esz_in(c)) * px * filtersize, "pointwise input" },
                  { output, (lit ? 1.0 : esz_out(c)) * px * op_size, "pointwise output" },
                  { filter_k, (dtype == MBN_DT_BF16 ? 2.0 : 4.0) * op_size * filtersize +
                                  ((dtype == MBN_DT_BF16 && (c.io_flags & MBN_IO_FILT_PACKED)) ? (double)mbn_packed_filter_offset(op_size, filtersize) : 0.0),
                    "pointwise filter" },
                  { c.scale, 4.0 * op_size, "pointwise scale" }, { c.shift, 4.0 * op_size, "pointwise shift" });
    }
    Scope sc(ctx, c.stream);
    if (dtype == MBN_DT_U8)
        return sc.finish(mbn_launch_lit_pointwise(c, (uint8_t *)output, (const uint8_t *)inp_image,
                                                  (const int32_t *)filter_k, rows, cols, filtersize, op_size));
    long m = (long)c.batch * rows * cols;
    return sc.finish(mbn_launch_f32_pointwise(c, output, inp_image, filter_k, m, filtersize, op_size));
}

int mbn_pool(mbn_context *ctx, void *output, const void *inp_image, int rows, int cols, int filtersize, int op_size,
             const mbn_layer_ext *ext)
{
    mbn_call c;
    int dtype;
    int rc = resolve(ctx, ext, &c, &dtype);
    if (rc != MBN_OK) return rc;
    if (!output || !inp_image) return MBN_EINVAL;
    if (rows <= 0 || cols <= 0 || op_size <= 0 || filtersize <= 0) return MBN_EINVAL;
    if (dtype == MBN_DT_U8 && (long)filtersize * filtersize > (long)rows * cols) return MBN_EINVAL;   // kernel.cl:126 would run past the plane
    if (dtype == MBN_DT_I8) {
        if (c.io_flags & MBN_IO_OUT_F32) return MBN_EUNSUPPORTED;
        if (op_size % 8 || (uintptr_t)output % 8 || (uintptr_t)inp_image % 8) return MBN_EUNSUPPORTED;   // no mult / bias, any act
        MBN_SPANS(ctx, { inp_image, 1.0 * c.batch * rows * cols * op_size, "pool input" }, { output, 1.0 * c.batch * op_size, "pool output" });
        Scope sc(ctx, c.stream);
        return sc.finish(mbn_launch_i8_pool(c, (uint8_t *)output, (const uint8_t *)inp_image, rows, cols, filtersize, op_size));
    }
    {
        const double lit = dtype == MBN_DT_U8;
        MBN_SPANS(ctx, { inp_image, (lit ? 1.0 : esz_in(c)) * c.batch * rows * cols * op_size, "pool input" },
                  { output, (lit ? 1.0 : esz_out(c)) * c.batch * op_size, "pool output" });
    }
    Scope sc(ctx, c.stream);
    if (dtype == MBN_DT_U8) {
        return sc.finish(mbn_launch_lit_pool(c, (uint8_t *)output, (const uint8_t *)inp_image, rows, cols, filtersize,
                                             op_size));
    }
    return sc.finish(mbn_launch_f32_pool(c, output, inp_image, rows, cols, filtersize, op_size));
}

int mbn_softmax_f32(mbn_context *ctx, void *probs, void *argmax_i32, const void *logits, int batch, int classes,
                    void *stream)
{
    if (!ctx || !logits || batch <= 0 || classes <= 0 || (!probs && !argmax_i32)) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { logits, 4.0 * batch * classes, "softmax logits" }, { probs, 4.0 * batch * classes, "softmax probs" },
              { argmax_i32, 4.0 * batch, "softmax argmax" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_softmax(ctx, s, (float *)probs, (int32_t *)argmax_i32, (const float *)logits, batch,
                                            classes));
}

int mbn_softmax_topk_f32(mbn_context *ctx, void *probs, void *topk_idx_i32, void *topk_prob_f32, const void *logits,
                         int batch, int classes, int k, void *stream)
{
    if (!ctx || !logits || !topk_idx_i32 || !topk_prob_f32 || batch <= 0 || classes <= 0 || k < 1 || k > 8) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { logits, 4.0 * batch * classes, "softmax_topk logits" }, { probs, 4.0 * batch * classes, "softmax_topk probs" },
              { topk_idx_i32, 4.0 * batch * k, "softmax_topk idx" }, { topk_prob_f32, 4.0 * batch * k, "softmax_topk prob" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_softmax_topk(ctx, s, (float *)probs, (int32_t *)topk_idx_i32, (float *)topk_prob_f32,
                                                 (const float *)logits, batch, classes, k));
}

int mbn_upsample_argmax_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                            int factor, void *stream)
{
    if (!ctx || !labels_i32 || !logits || batch <= 0 || rows <= 0 || cols <= 0 || classes <= 0) return MBN_EINVAL;
    if (((uintptr_t)labels_i32 | (uintptr_t)score_f32 | (uintptr_t)logits) % 4) return MBN_EINVAL;
    if (mbn_upsample_argmax_envelope(batch, rows, cols, classes, factor) != MBN_OK) return MBN_EUNSUPPORTED;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const double out = 4.0 * batch * rows * factor * cols * factor;
    MBN_SPANS(ctx, { logits, 4.0 * batch * rows * cols * classes, "upsample_argmax logits" }, { labels_i32, out, "upsample_argmax labels" },
              { score_f32, out, "upsample_argmax score" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_upsample_argmax(ctx, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, batch, rows, cols,
                                                    classes, factor));
}

// What the six read-outs at any output size share. q = null is mbn_resample_argmax_*, q given mbn_resample_softmax_* (whose own argument checks,
// prob's alignment and mbn_softmax_readout_check, come with the pointers', in front of the shape). shape: what the call's own envelope answered;
// out_bytes: what the launch reaches of labels, score and prob each; launch(s) enqueues it on the stream chosen here.
extern "C++" {
template <typename Launch>
static int readout_call(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, const mbn_readout_prob *q, int shape,
                        double logits_bytes, double out_bytes, void *stream, Launch launch)
{
    if (!ctx || !labels_i32 || !logits) return MBN_EINVAL;
    if (((uintptr_t)labels_i32 | (uintptr_t)score_f32 | (uintptr_t)logits | (uintptr_t)(q ? q->prob : nullptr)) % 4) return MBN_EINVAL;
    if (q && mbn_softmax_readout_check(q->prob != nullptr, q->min_prob) != MBN_OK) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { logits, logits_bytes, "resample read-out logits" }, { labels_i32, out_bytes, "resample read-out labels" },
              { score_f32, out_bytes, "resample read-out score" }, { q ? q->prob : nullptr, out_bytes, "resample read-out prob" });
    Scope sc(ctx, s);
    return sc.finish(launch(s));
}
}   // extern "C++"

// rect = null: the whole map, mbn_resample_argmax_f32 / _softmax_f32 (window = false: a null rect of the window calls is their envelope's to refuse)
static int resample_uniform(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                            bool window, int in_rows, int in_cols, const int32_t *rect, int out_rows, int out_cols, void *stream,
                            const mbn_readout_prob *q)
{
    const int shape = window ? mbn_resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols)
                             : mbn_resample_argmax_envelope(batch, rows, cols, classes, out_rows, out_cols);
    return readout_call(ctx, labels_i32, score_f32, logits, q, shape, 4.0 * batch * rows * cols * classes, 4.0 * batch * out_rows * out_cols, stream,
                        [&](hipStream_t s) {
                            return mbn_launch_f32_resample_argmax(ctx, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, batch, rows,
                                                                  cols, classes, in_rows, in_cols, rect, out_rows, out_cols, q);
                        });
}

int mbn_resample_argmax_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                            int out_rows, int out_cols, void *stream)
{
    return resample_uniform(ctx, labels_i32, score_f32, logits, batch, rows, cols, classes, false, 0, 0, nullptr, out_rows, out_cols, stream, nullptr);
}

int mbn_resample_softmax_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                             int classes, int out_rows, int out_cols, float min_prob, int ignore_label, void *stream)
{
    const mbn_readout_prob q = { (float *)prob_f32, min_prob, ignore_label };
    return resample_uniform(ctx, labels_i32, score_f32, logits, batch, rows, cols, classes, false, 0, 0, nullptr, out_rows, out_cols, stream, &q);
}

int mbn_resample_argmax_window_f32(mbn_context *ctx, void *labels_i32, void *score_f32, const void *logits, int batch, int rows, int cols, int classes,
                                   int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols, void *stream)
{
    return resample_uniform(ctx, labels_i32, score_f32, logits, batch, rows, cols, classes, true, in_rows, in_cols, rect, out_rows, out_cols, stream,
                            nullptr);
}

int mbn_resample_softmax_window_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows,
                                    int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                                    float min_prob, int ignore_label, void *stream)
{
    const mbn_readout_prob q = { (float *)prob_f32, min_prob, ignore_label };
    return resample_uniform(ctx, labels_i32, score_f32, logits, batch, rows, cols, classes, true, in_rows, in_cols, rect, out_rows, out_cols, stream, &q);
}

int mbn_resample_ensemble_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                              int classes, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols, float min_prob,
                              int ignore_label, void *stream)
{
    if (!views || n_views < 1 || n_views > MBN_ENSEMBLE_MAX_VIEWS) return MBN_EINVAL;
    // no prob map and no threshold: the argmax form (a NaN threshold is not 0: the softmax check refuses it)
    const mbn_readout_prob prob = { (float *)prob_f32, min_prob, ignore_label };
    const mbn_readout_prob *q = prob_f32 || !(min_prob == 0.0f) ? &prob : nullptr;
    const int shape = mbn_resample_ensemble_envelope(batch, rows, cols, classes, in_rows, in_cols, views, n_views, out_rows, out_cols);
    return readout_call(ctx, labels_i32, score_f32, logits, q, shape, 4.0 * n_views * batch * rows * cols * classes, 4.0 * batch * out_rows * out_cols,
                        stream, [&](hipStream_t s) {
                            return mbn_launch_f32_resample_ensemble(ctx, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, batch,
                                                                    rows, cols, classes, in_rows, in_cols, views, n_views, out_rows, out_cols, q);
                        });
}

int mbn_resample_slide_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                           int classes, const mbn_slide *plan, int out_rows, int out_cols, float min_prob, int ignore_label, void *stream)
{
    if (!plan) return MBN_EINVAL;
    // no prob map and no threshold: the argmax form (a NaN threshold is not 0: the softmax check refuses it)
    const mbn_readout_prob prob = { (float *)prob_f32, min_prob, ignore_label };
    const mbn_readout_prob *q = prob_f32 || !(min_prob == 0.0f) ? &prob : nullptr;
    const int shape = mbn_resample_slide_envelope(batch, rows, cols, classes, plan, out_rows, out_cols);
    const double maps = shape == MBN_OK ? (double)batch * plan->ny * plan->nx : 0.0;
    return readout_call(ctx, labels_i32, score_f32, logits, q, shape, 4.0 * maps * rows * cols * classes, 4.0 * batch * out_rows * out_cols, stream,
                        [&](hipStream_t s) {
                            return mbn_launch_f32_resample_slide(ctx, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, batch, rows,
                                                                 cols, classes, plan, out_rows, out_cols, q);
                        });
}

int mbn_ragged_readout_create(mbn_context *ctx, int max_batch, mbn_ragged_readout **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    if (max_batch <= 0) return MBN_EINVAL;
    if (max_batch > MBN_DENSE_MAX_BATCH) return MBN_EUNSUPPORTED;
    const int rc = mbn_ragged_readout_build(ctx, max_batch, r);
    if (rc != MBN_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->ragged_readouts.push_back(*r);
    return MBN_OK;
}

int mbn_ragged_readout_destroy(mbn_ragged_readout *r)
{
    if (!r) return MBN_OK;
    mbn_context *ctx = r->ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto it = ctx->ragged_readouts.begin(); it != ctx->ragged_readouts.end(); ++it)
            if (*it == r) { ctx->ragged_readouts.erase(it); break; }
    }
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipEventSynchronize(r->done));              // its last upload or launch, whatever the stream
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mbn_ragged_readout_release(r);
    return MBN_OK;
}

int mbn_ragged_readout_set(mbn_ragged_readout *r, int rows, int cols, int classes, const mbn_label_item *items, int batch, void *stream)
{
    if (!r || !items || batch <= 0 || batch > r->max_batch || rows <= 0 || cols <= 0 || classes <= 0) return MBN_EINVAL;
    mbn_context *ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    return mbn_ragged_readout_plan(r, stream ? (hipStream_t)stream : ctx->stream, rows, cols, classes, 0, 0, 0, items, batch);
}

int mbn_ragged_readout_set_window(mbn_ragged_readout *r, int rows, int cols, int classes, int in_rows, int in_cols,
                                  const mbn_label_window_item *items, int batch, void *stream)
{
    if (!r || !items || batch <= 0 || batch > r->max_batch || rows <= 0 || cols <= 0 || classes <= 0 || in_rows <= 0 || in_cols <= 0) return MBN_EINVAL;
    mbn_context *ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    return mbn_ragged_readout_plan(r, stream ? (hipStream_t)stream : ctx->stream, rows, cols, classes, 1, in_rows, in_cols, items, batch);
}

static int resample_ragged(mbn_ragged_readout *r, void *labels_i32, void *score_f32, const void *logits, void *stream, const mbn_readout_prob *q)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to launch
    return readout_call(r->ctx, labels_i32, score_f32, logits, q, MBN_OK, 4.0 * r->batch * r->rows * r->cols * r->classes, 4.0 * (double)r->launch.span,
                        stream, [&](hipStream_t s) {
                            return mbn_launch_f32_resample_argmax_ragged(r, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, q);
                        });
}

int mbn_resample_argmax_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *score_f32, const void *logits, void *stream)
{
    return resample_ragged(r, labels_i32, score_f32, logits, stream, nullptr);
}

int mbn_resample_softmax_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, float min_prob,
                                    int ignore_label, void *stream)
{
    const mbn_readout_prob q = { (float *)prob_f32, min_prob, ignore_label };
    return resample_ragged(r, labels_i32, score_f32, logits, stream, &q);
}

// The top-k read-outs: readout_call with the k rank-major planes as the outputs' span. No prob map and no threshold: the logit form (q = null; a NaN
// threshold is not 0: the softmax check refuses it), the ensemble's convention
int mbn_resample_topk_f32(mbn_context *ctx, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int batch, int rows, int cols,
                          int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols, int k, float min_prob,
                          int ignore_label, void *stream)
{
    const mbn_readout_prob prob = { (float *)prob_f32, min_prob, ignore_label };
    const mbn_readout_prob *q = prob_f32 || !(min_prob == 0.0f) ? &prob : nullptr;
    const int shape = mbn_resample_topk_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols, k);
    return readout_call(ctx, labels_i32, score_f32, logits, q, shape, 4.0 * batch * rows * cols * classes, 4.0 * k * batch * out_rows * out_cols, stream,
                        [&](hipStream_t s) {
                            return mbn_launch_f32_resample_topk(ctx, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, batch, rows,
                                                                cols, classes, in_rows, in_cols, rect, out_rows, out_cols, k, q);
                        });
}

int mbn_resample_topk_ragged_f32(mbn_ragged_readout *r, void *labels_i32, void *prob_f32, void *score_f32, const void *logits, int k,
                                 int64_t plane_stride, float min_prob, int ignore_label, void *stream)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to launch
    const mbn_readout_prob prob = { (float *)prob_f32, min_prob, ignore_label };
    const mbn_readout_prob *q = prob_f32 || !(min_prob == 0.0f) ? &prob : nullptr;
    const int shape = mbn_resample_topk_ragged_check(r->classes, r->launch.span, k, plane_stride);
    const double out_bytes = shape == MBN_OK ? 4.0 * ((double)(k - 1) * (double)plane_stride + (double)r->launch.span) : 0.0;
    return readout_call(r->ctx, labels_i32, score_f32, logits, q, shape, 4.0 * r->batch * r->rows * r->cols * r->classes, out_bytes, stream,
                        [&](hipStream_t s) {
                            return mbn_launch_f32_resample_topk_ragged(r, s, (int32_t *)labels_i32, (float *)score_f32, (const float *)logits, k,
                                                                       plane_stride, q);
                        });
}

// What the two NLL read-outs share: the pointer and alignment checks and the temperatures (MBN_EINVAL) in front of the shape's limits, the spans
// (`span` elements of truth and of one plane of each map, `plane` elements from plane to plane), the launch
extern "C++" {
template <typename Launch>
static int nll_call(mbn_context *ctx, void *nll_u64, void *nll_f32, void *brier_f32, const void *logits, const void *truth, int truth_bytes,
                    int classes, const float *inv_temps, int temps, int shape, double logits_bytes, double span, double plane, void *stream,
                    Launch launch)
{
    if (!ctx || !nll_u64 || !logits || !truth || !inv_temps || shape == MBN_EINVAL) return MBN_EINVAL;
    if ((uintptr_t)nll_u64 % 8 || ((uintptr_t)nll_f32 | (uintptr_t)brier_f32 | (uintptr_t)logits) % 4 || (truth_bytes == 4 && (uintptr_t)truth % 4))
        return MBN_EINVAL;
    if (mbn_nll_temps_check(inv_temps, temps) != MBN_OK) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const double map_bytes = 4.0 * ((double)(temps - 1) * plane + span);
    MBN_SPANS(ctx, { nll_u64, 32.0 * temps * (classes + 1), "nll table" }, { nll_f32, map_bytes, "nll map" }, { brier_f32, map_bytes, "brier map" },
              { logits, logits_bytes, "nll logits" }, { truth, (double)truth_bytes * span, "nll truth" });
    Scope sc(ctx, s);
    return sc.finish(launch(s));
}
}   // extern "C++"

int mbn_resample_nll_f32(mbn_context *ctx, void *nll_u64, void *nll_f32, void *brier_f32, const void *logits, const void *truth, int truth_bytes,
                         int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                         const float *inv_temps, int temps, void *stream)
{
    const int shape = mbn_resample_nll_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols, truth_bytes, temps);
    const double span = shape == MBN_OK ? (double)batch * out_rows * out_cols : 0.0;
    return nll_call(ctx, nll_u64, nll_f32, brier_f32, logits, truth, truth_bytes, classes, inv_temps, temps, shape,
                    4.0 * batch * rows * cols * classes, span, span, stream, [&](hipStream_t s) {
                        return mbn_launch_f32_resample_nll(ctx, s, nll_u64, (float *)nll_f32, (float *)brier_f32, (const float *)logits, truth,
                                                           truth_bytes, batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols,
                                                           inv_temps, temps);
                    });
}

int mbn_resample_nll_ragged_f32(mbn_ragged_readout *r, void *nll_u64, void *nll_f32, void *brier_f32, int64_t plane_stride, const void *logits,
                                const void *truth, int truth_bytes, const float *inv_temps, int temps, void *stream)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to score
    const int shape = mbn_resample_nll_ragged_check(r->classes, r->launch.span, truth_bytes, temps, plane_stride);
    return nll_call(r->ctx, nll_u64, nll_f32, brier_f32, logits, truth, truth_bytes, r->classes, inv_temps, temps, shape,
                    4.0 * r->batch * r->rows * r->cols * r->classes, (double)r->launch.span, (double)plane_stride, stream, [&](hipStream_t s) {
                        return mbn_launch_f32_resample_nll_ragged(r, s, nll_u64, (float *)nll_f32, (float *)brier_f32, plane_stride,
                                                                  (const float *)logits, truth, truth_bytes, inv_temps, temps);
                    });
}

// What the two rank-score calls share: confusion_call's checks with the rank table and the k label planes
extern "C++" {
template <typename Launch>
static int topk_rank_call(mbn_context *ctx, void *ranks_u64, const void *labels_i32, int k, int64_t plane_stride, const void *truth, int truth_bytes,
                          int classes, int64_t elements, void *stream, Launch launch)
{
    if (!ctx || !ranks_u64 || !labels_i32 || !truth) return MBN_EINVAL;
    const int shape = mbn_topk_rank_envelope(classes, truth_bytes, elements, k, plane_stride);
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)ranks_u64 % 8 || (uintptr_t)labels_i32 % 4 || (truth_bytes == 4 && (uintptr_t)truth % 4)) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { ranks_u64, 8.0 * (classes + 1) * (k + 1), "topk_rank ranks" },
              { labels_i32, 4.0 * ((double)(k - 1) * (double)plane_stride + (double)elements), "topk_rank labels" },
              { truth, (double)truth_bytes * (double)elements, "topk_rank truth" });
    Scope sc(ctx, s);
    return sc.finish(launch(s));
}
}   // extern "C++"

int mbn_topk_rank_i32(mbn_context *ctx, void *ranks_u64, const void *labels_i32, int k, int64_t plane_stride, const void *truth, int truth_bytes,
                      int classes, int64_t count, void *stream)
{
    return topk_rank_call(ctx, ranks_u64, labels_i32, k, plane_stride, truth, truth_bytes, classes, count, stream, [&](hipStream_t s) {
        return mbn_launch_i32_topk_rank(ctx, s, ranks_u64, labels_i32, k, plane_stride, truth, truth_bytes, classes, count);
    });
}

int mbn_topk_rank_ragged_i32(mbn_ragged_readout *r, void *ranks_u64, const void *labels_i32, int k, int64_t plane_stride, const void *truth,
                             int truth_bytes, int classes, void *stream)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to score
    return topk_rank_call(r->ctx, ranks_u64, labels_i32, k, plane_stride, truth, truth_bytes, classes, r->launch.span, stream, [&](hipStream_t s) {
        return mbn_launch_i32_topk_rank_ragged(r, s, ranks_u64, labels_i32, k, plane_stride, truth, truth_bytes, classes);
    });
}

// What the two calibration calls share: confusion_call's checks with the table of bins and the probability map beside the labels
extern "C++" {
template <typename Launch>
static int calibration_call(mbn_context *ctx, void *calib_u64, const void *labels_i32, const void *prob_f32, const void *truth, int truth_bytes,
                            int classes, int bins, int64_t elements, void *stream, Launch launch)
{
    if (!ctx || !calib_u64 || !labels_i32 || !prob_f32 || !truth) return MBN_EINVAL;
    const int shape = mbn_calibration_envelope(classes, truth_bytes, bins, elements);
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)calib_u64 % 8 || (uintptr_t)labels_i32 % 4 || (uintptr_t)prob_f32 % 4 || (truth_bytes == 4 && (uintptr_t)truth % 4)) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { calib_u64, 32.0 * (bins + 1), "calibration table" }, { labels_i32, 4.0 * (double)elements, "calibration labels" },
              { prob_f32, 4.0 * (double)elements, "calibration prob" }, { truth, (double)truth_bytes * (double)elements, "calibration truth" });
    Scope sc(ctx, s);
    return sc.finish(launch(s));
}
}   // extern "C++"

int mbn_calibration_f32(mbn_context *ctx, void *calib_u64, const void *labels_i32, const void *prob_f32, const void *truth, int truth_bytes,
                        int classes, int bins, int64_t count, void *stream)
{
    return calibration_call(ctx, calib_u64, labels_i32, prob_f32, truth, truth_bytes, classes, bins, count, stream, [&](hipStream_t s) {
        return mbn_launch_f32_calibration(ctx, s, calib_u64, labels_i32, prob_f32, truth, truth_bytes, classes, bins, count);
    });
}

int mbn_calibration_ragged_f32(mbn_ragged_readout *r, void *calib_u64, const void *labels_i32, const void *prob_f32, const void *truth,
                               int truth_bytes, int classes, int bins, void *stream)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to score
    return calibration_call(r->ctx, calib_u64, labels_i32, prob_f32, truth, truth_bytes, classes, bins, r->launch.span, stream, [&](hipStream_t s) {
        return mbn_launch_f32_calibration_ragged(r, s, calib_u64, labels_i32, prob_f32, truth, truth_bytes, classes, bins);
    });
}

// What the two confusion calls share: the pointer and alignment checks, the envelope, the spans (`elements` of labels and truth), the launch
extern "C++" {
template <typename Launch>
static int confusion_call(mbn_context *ctx, void *counts_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes, int64_t elements,
                          void *stream, Launch launch)
{
    if (!ctx || !counts_u64 || !labels_i32 || !truth) return MBN_EINVAL;
    const int shape = mbn_confusion_envelope(classes, truth_bytes, elements);
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)counts_u64 % 8 || (uintptr_t)labels_i32 % 4 || (truth_bytes == 4 && (uintptr_t)truth % 4)) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { counts_u64, 8.0 * (classes + 1) * (classes + 1), "confusion counts" }, { labels_i32, 4.0 * (double)elements, "confusion labels" },
              { truth, (double)truth_bytes * (double)elements, "confusion truth" });
    Scope sc(ctx, s);
    return sc.finish(launch(s));
}
}   // extern "C++"

int mbn_confusion_i32(mbn_context *ctx, void *counts_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes, int64_t count,
                      void *stream)
{
    return confusion_call(ctx, counts_u64, labels_i32, truth, truth_bytes, classes, count, stream, [&](hipStream_t s) {
        return mbn_launch_i32_confusion(ctx, s, counts_u64, labels_i32, truth, truth_bytes, classes, count);
    });
}

int mbn_confusion_ragged_i32(mbn_ragged_readout *r, void *counts_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes,
                             void *stream)
{
    if (!r || r->batch <= 0) return MBN_EINVAL;                  // no set: nothing to score
    return confusion_call(r->ctx, counts_u64, labels_i32, truth, truth_bytes, classes, r->launch.span, stream, [&](hipStream_t s) {
        return mbn_launch_i32_confusion_ragged(r, s, counts_u64, labels_i32, truth, truth_bytes, classes);
    });
}

int mbn_resizer_create_filter(mbn_context *ctx, int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resizer **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    int rc = mbn_resize_envelope_filter(filter, in_rows, in_cols, box, out_rows, out_cols);
    if (rc != MBN_OK) return rc;
    rc = mbn_resizer_build(ctx, filter, in_rows, in_cols, box, out_rows, out_cols, false, r);
    if (rc != MBN_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->resizers.push_back(*r);
    return MBN_OK;
}

int mbn_resizer_create(mbn_context *ctx, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resizer **r)
{
    return mbn_resizer_create_filter(ctx, MBN_FILTER_BILINEAR, in_rows, in_cols, box, out_rows, out_cols, r);
}

int mbn_resizer_create_pad(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const uint8_t fill[3], mbn_resizer **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    if (!fill) return MBN_EINVAL;
    const int rc = mbn_resizer_build_pad(ctx, filter, in_rows, in_cols, out_rows, out_cols, fill, r);      // the plan answers for the geometry
    if (rc != MBN_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->resizers.push_back(*r);
    return MBN_OK;
}

int mbn_resizer_create_view(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view,
                            const uint8_t fill[3], mbn_resizer **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    if (!view || !fill) return MBN_EINVAL;
    const int rc = mbn_resizer_build_view(ctx, filter, in_rows, in_cols, out_rows, out_cols, view, fill, r);       // the plan answers for the geometry
    if (rc != MBN_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->resizers.push_back(*r);
    return MBN_OK;
}

int mbn_resizer_destroy(mbn_resizer *r)
{
    if (!r) return MBN_OK;
    mbn_context *ctx = r->ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto it = ctx->resizers.begin(); it != ctx->resizers.end(); ++it)
            if (*it == r) { ctx->resizers.erase(it); break; }
    }
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mbn_resizer_release(r);
    return MBN_OK;
}

int mbn_resize_u8(mbn_resizer *r, void *out_u8, const void *in_u8, int batch, void *stream)
{
    if (!r || !out_u8 || !in_u8 || batch <= 0) return MBN_EINVAL;
    if (batch > MBN_RESIZE_MAX_BATCH) return MBN_EUNSUPPORTED;
    mbn_context *ctx = r->ctx;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { in_u8, 3.0 * batch * r->in_rows * r->in_cols, "resize_u8 in" }, { out_u8, 3.0 * batch * r->canvas_rows * r->canvas_cols, "resize_u8 out" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_u8_resize(r, s, (uint8_t *)out_u8, (const uint8_t *)in_u8, batch));
}

// fill: NULL for the plain handle, the border's colour for a letterbox
static int ragged_resizer_create(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, const uint8_t *fill, mbn_ragged_resizer **r)
{
    if (filter < MBN_FILTER_NEAREST || filter > MBN_FILTER_HAMMING || max_batch <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    if (filter == MBN_FILTER_HAMMING || filter == MBN_FILTER_LANCZOS) return MBN_EUNSUPPORTED;       // no device form of their weights (mbn.h)
    if (max_batch > MBN_RESIZE_MAX_BATCH || out_rows > MBN_RESIZE_MAX_OUT || out_cols > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;
    const int rc = mbn_ragged_resizer_build(ctx, filter, max_batch, out_rows, out_cols, fill, r);
    if (rc != MBN_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->ragged_resizers.push_back(*r);
    return MBN_OK;
}

int mbn_ragged_resizer_create_filter(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, mbn_ragged_resizer **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    return ragged_resizer_create(ctx, filter, max_batch, out_rows, out_cols, nullptr, r);
}

int mbn_ragged_resizer_create_pad(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, const uint8_t fill[3], mbn_ragged_resizer **r)
{
    if (!ctx || !r) return MBN_EINVAL;
    *r = nullptr;
    if (!fill) return MBN_EINVAL;
    return ragged_resizer_create(ctx, filter, max_batch, out_rows, out_cols, fill, r);
}

int mbn_ragged_resizer_create(mbn_context *ctx, int max_batch, int out_rows, int out_cols, mbn_ragged_resizer **r)
{
    return mbn_ragged_resizer_create_filter(ctx, MBN_FILTER_BILINEAR, max_batch, out_rows, out_cols, r);
}

int mbn_ragged_resizer_destroy(mbn_ragged_resizer *r)
{
    if (!r) return MBN_OK;
    mbn_context *ctx = r->ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto it = ctx->ragged_resizers.begin(); it != ctx->ragged_resizers.end(); ++it)
            if (*it == r) { ctx->ragged_resizers.erase(it); break; }
    }
    (void)hipSetDevice(ctx->device);
    MBN_HIP_TRY(ctx, hipEventSynchronize(r->done));              // its last upload or launch, whatever the stream
    MBN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mbn_ragged_resizer_release(r);
    return MBN_OK;
}

int mbn_ragged_resizer_set(mbn_ragged_resizer *r, const mbn_resize_item *items, int batch, void *stream)
{
    if (!r) return MBN_EINVAL;
    r->batch = 0;                                                // a failed set leaves the handle without a batch
    if (!items || batch <= 0 || batch > r->max_batch) return MBN_EINVAL;
    mbn_context *ctx = r->ctx;
    (void)hipSetDevice(ctx->device);
    return mbn_ragged_resizer_plan(r, stream ? (hipStream_t)stream : ctx->stream, items, batch);
}

int mbn_resize_ragged_u8(mbn_ragged_resizer *r, void *out_u8, const void *src_u8, void *stream)
{
    if (!r || !out_u8 || !src_u8 || r->batch <= 0) return MBN_EINVAL;
    mbn_context *ctx = r->ctx;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { src_u8, (double)r->src_span, "resize_ragged_u8 src" }, { out_u8, 3.0 * r->batch * r->out_rows * r->out_cols, "resize_ragged_u8 out" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_u8_resize_ragged(r, s, (uint8_t *)out_u8, (const uint8_t *)src_u8));
}

int mbn_resize_taps_device(mbn_context *ctx, int in_size, float b0, float b1, int out_size, void *first_i32, void *count_i32, void *weights_i32)
{
    return mbn_resize_taps_device_filter(ctx, MBN_FILTER_BILINEAR, in_size, b0, b1, out_size, first_i32, count_i32, weights_i32);
}

int mbn_resize_taps_device_filter(mbn_context *ctx, int filter, int in_size, float b0, float b1, int out_size, void *first_i32, void *count_i32,
                                  void *weights_i32)
{
    if (!ctx || !first_i32 || !count_i32 || !weights_i32) return MBN_EINVAL;
    if (((uintptr_t)first_i32 | (uintptr_t)count_i32 | (uintptr_t)weights_i32) % 4) return MBN_EINVAL;
    const int ksize = mbn_resize_ksize_filter(filter, in_size, b0, b1, out_size);
    if (ksize == MBN_EINVAL) return MBN_EINVAL;
    if (filter == MBN_FILTER_HAMMING || filter == MBN_FILTER_LANCZOS) return MBN_EUNSUPPORTED;       // no device form of their weights (mbn.h)
    if (ksize < 0 || ksize > MBN_RESIZE_MAX_KSIZE || in_size > MBN_RESIZE_MAX_IN || out_size > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;
    MBN_SPANS(ctx, { first_i32, 4.0 * out_size, "resize_taps_device first" }, { count_i32, 4.0 * out_size, "resize_taps_device count" },
              { weights_i32, 4.0 * out_size * ksize, "resize_taps_device weights" });
    Scope sc(ctx, ctx->stream);
    const int rc = sc.finish(mbn_launch_resize_taps(ctx->stream, filter, in_size, b0, b1, out_size, ksize, (int32_t *)first_i32, (int32_t *)count_i32,
                                                    (int32_t *)weights_i32));
    return rc == MBN_OK ? ksize : rc;
}

int mbn_classifier_tail(mbn_context *ctx, void *topk_idx_i32, void *topk_prob_f32, void *probs, void *logits_scratch,
                        void *pooled_scratch, const void *in, const void *fc_w, const void *fc_bias, int batch, int rows,
                        int cols, int channels, int classes, int k, void *stream)
{
    if (!ctx || !topk_idx_i32 || !topk_prob_f32 || !logits_scratch || !pooled_scratch || !in || !fc_w || batch <= 0 ||
        rows <= 0 || rows != cols || channels <= 0 || classes <= 0 || k < 1 || k > 8)
        return MBN_EINVAL;
    mbn_layer_ext e;
    memset(&e, 0, sizeof e);
    e.struct_size = sizeof e;
    e.batch = batch;
    e.dtype = MBN_DT_F32;
    e.layout = MBN_LAYOUT_NHWC;
    e.act = MBN_ACT_NONE;
    e.pad_top = e.pad_left = -1;
    e.stream = stream;
    int rc = mbn_pool(ctx, pooled_scratch, in, rows, cols, rows, channels, &e);           // MobileNet.c:2603-2656
    if (rc != MBN_OK) return rc;
    e.shift = fc_bias;                                                                     // bias, no ReLU (B15)
    rc = mbn_pointwise(ctx, logits_scratch, pooled_scratch, fc_w, 1, 1, channels, classes, &e);   // MobileNet.c:2682-2739
    if (rc != MBN_OK) return rc;
    return mbn_softmax_topk_f32(ctx, probs, topk_idx_i32, topk_prob_f32, logits_scratch, batch, classes, k, stream);
}

size_t mbn_pool_fc_workspace_bytes(int channels, int classes)
{
    if (channels < 64 || channels > 1024 || (channels % 64) != 0 || classes <= 0) return 0;
    return mbn_pool_fc_ws_bytes(channels, classes);
}

int mbn_pool_fc(mbn_context *ctx, void *logits, const void *in, const void *fc_w, const void *fc_bias, int batch, int rows, int cols,
                int channels, int classes, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ctx || !logits || !in || !fc_w || !workspace || batch <= 0 || rows <= 0 || cols <= 0 || channels <= 0 || classes <= 0) return MBN_EINVAL;
    if (batch > 4 || channels < 64 || channels > 1024 || (channels % 64) != 0) return MBN_EUNSUPPORTED;
    if (workspace_bytes < mbn_pool_fc_ws_bytes(channels, classes)) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { in, 4.0 * batch * rows * cols * channels, "pool_fc input" }, { logits, 4.0 * batch * classes, "pool_fc logits" },
              { fc_w, 4.0 * classes * channels, "pool_fc filter" }, { workspace, (double)mbn_pool_fc_ws_bytes(channels, classes), "pool_fc workspace" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_pool_fc(ctx, s, (float *)logits, (const float *)in, (const float *)fc_w, (const float *)fc_bias, workspace,
                                            batch, rows * cols, channels, classes, 0, nullptr, nullptr, nullptr));
}

int mbn_classifier_tail_fused(mbn_context *ctx, void *topk_idx_i32, void *topk_prob_f32, void *probs, void *logits, const void *in, const void *fc_w,
                              const void *fc_bias, int batch, int rows, int cols, int channels, int classes, int k, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    if (!ctx || !topk_idx_i32 || !topk_prob_f32 || !logits || !in || !fc_w || !workspace || batch <= 0 || rows <= 0 || cols <= 0 || channels <= 0 ||
        classes <= 0 || k < 1 || k > 8)
        return MBN_EINVAL;
    if (batch > 4 || channels < 64 || channels > 1024 || (channels % 64) != 0 || classes > 1024) return MBN_EUNSUPPORTED;
    if (workspace_bytes < mbn_pool_fc_ws_bytes(channels, classes)) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { in, 4.0 * batch * rows * cols * channels, "classifier_tail_fused input" }, { logits, 4.0 * batch * classes, "classifier_tail_fused logits" },
              { fc_w, 4.0 * classes * channels, "classifier_tail_fused filter" }, { workspace, (double)mbn_pool_fc_ws_bytes(channels, classes), "classifier_tail_fused workspace" },
              { probs, 4.0 * batch * classes, "classifier_tail_fused probs" }, { topk_idx_i32, 4.0 * batch * k, "classifier_tail_fused idx" },
              { topk_prob_f32, 4.0 * batch * k, "classifier_tail_fused prob" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_pool_fc(ctx, s, (float *)logits, (const float *)in, (const float *)fc_w, (const float *)fc_bias, workspace,
                                            batch, rows * cols, channels, classes, k, (float *)probs, (int32_t *)topk_idx_i32, (float *)topk_prob_f32));
}

static int stem_fused_impl(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                           const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                           int batch, int rows, int cols, int c1, int c3, void *stream, int in_u8, int bf16)
{
    if (!ctx || !out || !image) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // decide before opening the profiling scope so an unsupported shape does not consume an event slot
    if (mbn_stem_envelope_hw(batch, rows, cols, c1, c3) != MBN_OK) return MBN_EUNSUPPORTED;
    MBN_SPANS(ctx, { image, (in_u8 ? 1.0 : 4.0) * batch * rows * cols * 3, "stem image" },
              { out, (bf16 ? 2.0 : 4.0) * batch * (rows / 2) * (cols / 2) * c3, "stem output" });
    // parameters the kernel cannot load (null or off 16 bytes) are unsupported; an output off 16 bytes or an image off its load width is invalid
    if (check_ptrs({ w1, s1, b1, wd, s2, b2, wp, s3, b3 }) != MBN_OK) return MBN_EUNSUPPORTED;
    if (((uintptr_t)out % 16) != 0 || ((uintptr_t)image % (in_u8 ? 2 : 8)) != 0) return MBN_EINVAL;
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_f32_stem(ctx, s, (float *)out, (const float *)image, (const float *)w1, (const float *)s1,
                                         (const float *)b1, (const float *)wd, (const float *)s2, (const float *)b2,
                                         (const float *)wp, (const float *)s3, (const float *)b3, batch, rows, cols, c1, c3, in_u8, bf16));
}

int mbn_stem_fused_hw(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int rows, int cols, int c1, int c3, int flags, void *stream)
{
    if (flags & ~(MBN_STEM_IN_U8 | MBN_STEM_BF16)) return MBN_EINVAL;
    return stem_fused_impl(ctx, out, image, w1, s1, b1, wd, s2, b2, wp, s3, b3, batch, rows, cols, c1, c3, stream,
                           (flags & MBN_STEM_IN_U8) != 0, (flags & MBN_STEM_BF16) != 0);
}

int mbn_stem_fused(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                   const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                   int batch, int res, int c1, int c3, void *stream)
{
    return mbn_stem_fused_hw(ctx, out, image, w1, s1, b1, wd, s2, b2, wp, s3, b3, batch, res, res, c1, c3, 0, stream);
}

int mbn_stem_fused_u8(mbn_context *ctx, void *out, const void *image_u8, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int res, int c1, int c3, void *stream)
{
    return mbn_stem_fused_hw(ctx, out, image_u8, w1, s1, b1, wd, s2, b2, wp, s3, b3, batch, res, res, c1, c3, MBN_STEM_IN_U8, stream);
}

int mbn_stem_fused_ex(mbn_context *ctx, void *out, const void *image, const void *w1, const void *s1, const void *b1,
                      const void *wd, const void *s2, const void *b2, const void *wp, const void *s3, const void *b3,
                      int batch, int res, int c1, int c3, int flags, void *stream)
{
    return mbn_stem_fused_hw(ctx, out, image, w1, s1, b1, wd, s2, b2, wp, s3, b3, batch, res, res, c1, c3, flags, stream);
}

int mbn_dwpw_fused(mbn_context *ctx, void *out, const void *in, const void *wd, const void *s2, const void *b2,
                   const void *wp, const void *s3, const void *b3, int batch, int in_rows, int in_cols, int out_rows,
                   int out_cols, int cin, int cout, int stride, int pad_top, int pad_left, void *stream)
{
    if (!ctx) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const mbn_block_shape sh = { batch, in_rows, in_cols, out_rows, out_cols, cin, cout, stride, pad_top, pad_left };
    const mbn_block_params p = { wd, s2, b2, wp, s3, b3 };
    // decide before opening the profiling scope so an unsupported shape does not consume an event slot
    int rc = check_ptrs({ in, wd, s2, b2, wp, s3, b3, out });
    if (rc == MBN_OK) rc = mbn_block_envelope(&sh, MBN_DT_F32);
    if (rc != MBN_OK) return rc;
    MBN_SPANS(ctx, { in, 4.0 * batch * in_rows * in_cols * cin, "dwpw input" },
              { out, 4.0 * batch * out_rows * out_cols * cout, "dwpw output" }, { wd, 36.0 * cin, "dwpw depthwise filter" },
              { wp, 4.0 * cin * cout, "dwpw pointwise filter" });
    Scope sc(ctx, s);
    // unified-wave kernel (mbn_f32_dwpw2.hip) for the 128-column tile, where it measures 9-12 % faster than the round-1
    // producer/consumer kernel; the 256-column tile stays on the round-1 kernel (within +-3 % of each other there).
    // dwpw_variant: 1 = always round-1, 2 = always unified (A/B hooks, tools/block_bench.py)
    // small problems (few images): a 256-column tile leaves most CUs idle and every workgroup walks the whole K alone —
    // batch 1, block 10-11: 40 us fused against 24 us as two launches — so below one 256-wide tile per CU the block runs
    // on 128-column tiles (twice the workgroups, half the MFMA work per step), i.e. on the unified kernel
    // opt-in: pointwise products on the bf16 matrix cores from exact operand splits (mbn_f32_dwpw2_x6.hip; pw_emul = 6 | 9)
    if (g_mbn_tune.pw_emul != 0 && g_mbn_tune.dwpw_variant == 0 && mbn_launch_f32_dwpw2_x6(ctx, s, sh, out, in, p) == MBN_OK)
        return sc.finish(MBN_OK);
    const int dv = g_mbn_tune.dwpw_variant;
    // round 6: the wave-private form (mbn_f32_dwpw3.hip: no barrier in the loop, filter slice resident in LDS) where it applies
    // (Cin 64 / 128 / 256). Lab A/B: dwpw_variant 11 = always where eligible, 12 = never, 300 + bits = its ablation build.
    if ((dv == 11 || dv >= 300 || (dv == 0 && MBN_DWPW3_DEFAULT(stride, cin))) && mbn_f32_dwpw3_eligible(ctx, sh))
        return sc.finish(mbn_launch_f32_dwpw3(ctx, s, sh, out, in, p));
    const long tiles256 = (((long)batch * out_rows * out_cols + 127) / 128) * (cout / 256);
    const bool small = tiles256 < ctx->num_cus;
    // stride-2 blocks (15 x-window loads per lane and step): with the loads spread under the MFMA groups the unified kernel also wins at
    // 256 columns (block 8-9: 0.1967 / 0.1964 -> 0.1931 / 0.1893 ms, profiles/r02/b_block_kernel_variants.txt); stride 1 at 256 columns
    // stays on the round-1 kernel (block 10-11: 0.291 vs 0.308 ms)
    if (dv != 1 && (dv >= 2 || (cout % 256) != 0 || small || stride == 2))
        return sc.finish(mbn_launch_f32_dwpw2(ctx, s, sh, out, in, p));
    return sc.finish(mbn_launch_f32_dwpw(ctx, s, sh, out, in, p));
}

int mbn_blocks_resident_bf16(mbn_context *ctx, void *out, const void *in, const mbn_block_params *blocks, int nblocks, int batch,
                             int rows, int cols, int channels, void *stream)
{
    if (!ctx || !out || !in || !blocks || batch <= 0) return MBN_EINVAL;
    const mbn_block_shape sh = { batch, rows, cols, rows, cols, channels, channels, 1, 1, 1 };
    if (mbn_resident_envelope(&sh, nblocks) != MBN_OK) return MBN_EUNSUPPORTED;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const double act = 2.0 * batch * rows * cols * channels;
    MBN_SPANS(ctx, { in, act, "resident blocks input" }, { out, act, "resident blocks output" });
    for (int i = 0; i < nblocks; i++) {
        if (!blocks[i].wd || !blocks[i].s2 || !blocks[i].b2 || !blocks[i].wp_bf16 || !blocks[i].s3 || !blocks[i].b3) return MBN_EINVAL;
        MBN_SPANS(ctx, { blocks[i].wd, 36.0 * channels, "resident blocks depthwise filter" }, { blocks[i].wp_bf16, 2.0 * channels * channels, "resident blocks pointwise filter" },
                  { blocks[i].s2, 4.0 * channels, "resident blocks scale" }, { blocks[i].b3, 4.0 * channels, "resident blocks shift" });
    }
    int rc = check_ptrs({ out, in });
    for (int i = 0; i < nblocks && rc == MBN_OK; i++) rc = check_ptrs(blocks[i]);
    if (rc != MBN_OK) return rc;
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_bf16_res_blocks(ctx, s, out, in, blocks, nblocks, batch, rows, cols));
}

int mbn_tail_resident_bf16(mbn_context *ctx, void *out, const void *in, const mbn_block_params *blocks, int batch, int rows, int cols, int c0, int c1,
                           void *stream)
{
    if (!ctx || !out || !in || !blocks || batch <= 0) return MBN_EINVAL;
    const mbn_block_shape b0 = { batch, rows, cols, rows / 2, cols / 2, c0, c1, 2, 0, 0 };
    const mbn_block_shape b1 = { batch, rows / 2, cols / 2, rows / 2, cols / 2, c1, c1, 1, 1, 1 };
    if (mbn_tail_envelope(&b0, &b1) != MBN_OK) return MBN_EUNSUPPORTED;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { in, 2.0 * batch * rows * cols * c0, "resident tail input" }, { out, 2.0 * batch * c1, "resident tail output" });
    for (int i = 0; i < 2; i++) {
        if (!blocks[i].wd || !blocks[i].s2 || !blocks[i].b2 || !blocks[i].wp_bf16 || !blocks[i].s3 || !blocks[i].b3) return MBN_EINVAL;
        const int ci = i ? c1 : c0;
        MBN_SPANS(ctx, { blocks[i].wd, 36.0 * ci, "resident tail depthwise filter" }, { blocks[i].wp_bf16, 2.0 * ci * c1, "resident tail pointwise filter" },
                  { blocks[i].s2, 4.0 * ci, "resident tail scale" }, { blocks[i].b2, 4.0 * ci, "resident tail shift" },
                  { blocks[i].s3, 4.0 * c1, "resident tail scale" }, { blocks[i].b3, 4.0 * c1, "resident tail shift" });
    }
    int rc = ((uintptr_t)out % 2) ? MBN_EUNSUPPORTED : check_ptrs({ in });      // the pooled output is stored per bf16 element
    for (int i = 0; i < 2 && rc == MBN_OK; i++) rc = check_ptrs(blocks[i]);
    if (rc != MBN_OK) return rc;
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_bf16_tail(ctx, s, out, in, blocks, batch, rows, cols));
}

int mbn_dwpw_fused_bf16(mbn_context *ctx, void *out, const void *in, const void *wd, const void *s2, const void *b2,
                        const void *wp_bf16, const void *s3, const void *b3, int batch, int in_rows, int in_cols, int out_rows,
                        int out_cols, int cin, int cout, int stride, int pad_top, int pad_left, void *stream)
{
    if (!ctx) return MBN_EINVAL;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const mbn_block_shape sh = { batch, in_rows, in_cols, out_rows, out_cols, cin, cout, stride, pad_top, pad_left };
    const mbn_block_params p = { wd, s2, b2, wp_bf16, s3, b3 };
    int rc = check_ptrs({ in, wd, s2, b2, wp_bf16, s3, b3, out });
    if (rc == MBN_OK) rc = mbn_block_envelope(&sh, MBN_DT_BF16);
    if (rc != MBN_OK) return rc;
    MBN_SPANS(ctx, { in, 2.0 * batch * in_rows * in_cols * cin, "dwpw input" },
              { out, 2.0 * batch * out_rows * out_cols * cout, "dwpw output" }, { wd, 36.0 * cin, "dwpw depthwise filter" },
              { wp_bf16, 2.0 * cin * cout, "dwpw pointwise filter" });
    Scope sc(ctx, s);
#ifdef MBN_LAB
    if (g_mbn_tune.dwpw_variant == 1 && (cout % 128) == 0 && (cin % 64) == 0)      // the round-1 producer/consumer kernel (A/B hook; mbn_bf16_dwpw.hip's kernels are lab-only; whole 128-column tiles only)
        return sc.finish(mbn_launch_bf16_dwpw(ctx, s, sh, out, in, p));
#endif
    // unified-wave kernel (mbn_bf16_dwpw2.hip)
    return sc.finish(mbn_launch_bf16_dwpw2(ctx, s, sh, out, in, p));
}

int mbn_convert_f32_to_bf16(mbn_context *ctx, void *dst_bf16, const void *src_f32, size_t count, void *stream)
{
    if (!ctx || !dst_bf16 || !src_f32) return MBN_EINVAL;
    if (count == 0) return MBN_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { src_f32, 4.0 * count, "convert source" }, { dst_bf16, 2.0 * count, "convert destination" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_convert(ctx, s, dst_bf16, src_f32, count, 1));
}

size_t mbn_packed_filter_offset(int cout, int cin)
{
    if (cout <= 0 || cin <= 0 || (cout % 256) != 0 || (cin % 64) != 0) return 0;
    return ((size_t)cout * cin * 2 + 255) & ~(size_t)255;
}

int mbn_pack_filter_bf16(mbn_context *ctx, void *filter_buf, int cout, int cin, void *stream)
{
    if (!ctx || !filter_buf) return MBN_EINVAL;
    const size_t off = mbn_packed_filter_offset(cout, cin);
    if (off == 0) return MBN_EUNSUPPORTED;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { filter_buf, (double)off + 2.0 * cout * cin, "packed filter buffer" });
#ifdef MBN_LAB
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_pack_filter_bf16(ctx, s, (char *)filter_buf + off, filter_buf, cout, cin));
#else
    (void)s;
    return MBN_EUNSUPPORTED;           // the kernel that reads packed images is not part of the shipped library (see mbn.h)
#endif
}

int mbn_convert_bf16_to_f32(mbn_context *ctx, void *dst_f32, const void *src_bf16, size_t count, void *stream)
{
    if (!ctx || !dst_f32 || !src_bf16) return MBN_EINVAL;
    if (count == 0) return MBN_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { src_bf16, 2.0 * count, "convert source" }, { dst_f32, 4.0 * count, "convert destination" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_convert(ctx, s, dst_f32, src_bf16, count, 0));
}

int mbn_normalize_u8_to_f32(mbn_context *ctx, void *out_f32, const void *in_u8, size_t count, float scale, float bias,
                            void *stream)
{
    if (!ctx || !out_f32 || !in_u8) return MBN_EINVAL;
    if (count == 0) return MBN_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    MBN_SPANS(ctx, { in_u8, 1.0 * count, "normalize input" }, { out_f32, 4.0 * count, "normalize output" });
    Scope sc(ctx, s);
    return sc.finish(mbn_launch_normalize(ctx, s, (float *)out_f32, (const uint8_t *)in_u8, count, scale, bias));
}

}   // extern "C"
