// ctx.cpp -- contexts (one per GPU) and what every other unit of the host runtime stands on: memory that is freed
// without device-wide waits, the event pool, the per-stream state of batches, and the stream / event / copy wrappers
// of the C ABI.
#include "host.h"

namespace qpp {

// Memory without device-wide waits.  hipFree, hipHostFree, hipHostUnregister and hipDeviceSynchronize wait for EVERY
// stream of the device -- a resident server's too, and a server leaves only on its idle timeout (200 ms by default),
// or never while its flushes keep coming.  Measured beside a resident kernel (tools/diag/free_sync.hip,
// profiles/r05/r05v): each of those calls took 1950 ms next to a 2-s kernel; hipMalloc, hipHostMalloc, hipMallocAsync,
// hipFreeAsync, hipStreamDestroy and hipEventDestroy did not wait.  (The stream-ordered allocator was tried for device
// memory and corrupted batch buffers in the fuzz test -- 6-8 of 44 seeds, with or without device-wide synchronizes,
// 0 of 44 with hipMalloc / hipFree: profiles/r05/r05v/fuzzab.txt -- so it is not used.)  Hence:
//   * device and pinned buffers are freed at once only while no server of the device is resident (any context's,
//     this one's included), else parked in the device registry and freed by the next free, synchronize or destroy of
//     any context that finds none resident (release); parked memory is never reused before that hipFree, so work
//     still reading it is unaffected, and no server is stopped to free memory it does not read;
//   * a context's synchronize waits for every stream of the context (ctx_sync), never the device.
void hfree(qpp_ctx *ctx, void *p) { release(ctx, p, true); }
void dfree(qpp_ctx *ctx, void *p) {
    if (p) release(ctx, p, false);
}
void dfree_zeroed(qpp_ctx *ctx, void *p, size_t bytes) {
    if (!p) return;
    hipMemsetAsync(p, 0, bytes, ctx->stream);
    hipStreamSynchronize(ctx->stream);
    dfree(ctx, p);
}
// Sizes of the library's device and pinned allocations, so that release() counts parked bytes exactly (hipMemPtrGetInfo
// does not size every pinned buffer: ADVICE r5).  Process-wide: a buffer may be released by another context's call.
static std::mutex g_size_mu;
static std::unordered_map<void *, size_t> g_sizes;
void note_size(void *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_size_mu);
    g_sizes[p] = bytes;
}
size_t take_size(void *p) {
    std::lock_guard<std::mutex> lk(g_size_mu);
    auto it = g_sizes.find(p);
    if (it == g_sizes.end()) return 0;
    const size_t b = it->second;
    g_sizes.erase(it);
    return b;
}

hipEvent_t get_event(qpp_ctx *ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}
void put_event(qpp_ctx *ctx, hipEvent_t e) {
    if (e) ctx->event_pool.push_back(e);
}

// every stream the context's work runs on (the resident servers' excepted): its own, each batch stream's (with its
// ChaCha side stream, and the transmit queues' flush streams, which are batch streams), the host pipeline's
static std::vector<hipStream_t> ctx_streams(const qpp_ctx *ctx) {
    std::vector<hipStream_t> v;
    for (hipStream_t s : {ctx->stream, ctx->kstream, ctx->rstream})
        if (s) v.push_back(s);
    for (const StreamState *st : ctx->streams) {
        if (st->stream != ctx->stream) v.push_back(st->stream);
        if (st->side) v.push_back(st->side);
    }
    if (ctx->pipe)
        for (hipStream_t s : {ctx->pipe->h2d, ctx->pipe->comp, ctx->pipe->d2h})
            if (s) v.push_back(s);
    for (const qpp_txq *q : ctx->txqs)  // (zero-copy flushes run on them without a stream state; read the key table)
        for (hipStream_t s : q->streams) v.push_back(s);
    for (hipStream_t s : ctx->user_streams) v.push_back(s);
    return v;
}
// remember a caller's stream (see qpp_ctx::user_streams); returns it (NULL: the context stream)
static hipStream_t user_stream(qpp_ctx *ctx, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!s || s == ctx->stream) return ctx->stream;
    if (std::find(ctx->user_streams.begin(), ctx->user_streams.end(), s) == ctx->user_streams.end())
        ctx->user_streams.push_back(s);
    return s;
}
int ctx_sync(qpp_ctx *ctx) {
    for (hipStream_t s : ctx_streams(ctx)) HIP_TRY(ctx, hipStreamSynchronize(s));
    return QPP_OK;
}

void free_plan(qpp_ctx *ctx, PlanBuffers &p) {
    for (void *b : {(void *)p.counts, (void *)p.cursor, (void *)p.istart, (void *)p.perm, (void *)p.kq,
                    (void *)p.work, (void *)p.n_work})
        dfree(ctx, b);
    p = PlanBuffers{};
}
static void free_stream_state(qpp_ctx *ctx, StreamState *st) {
    hipStreamSynchronize(st->stream);
    if (st->side) hipStreamSynchronize(st->side);
    free_plan(ctx, st->plan);
    dfree(ctx, st->fips_buf);
    dfree(ctx, st->fips_refused);
    dfree(ctx, st->rx_scratch);
    if (st->side) hipStreamDestroy(st->side);
    if (st->fork_ev) hipEventDestroy(st->fork_ev);
    if (st->join_ev) hipEventDestroy(st->join_ev);
    if (st->last) hipEventDestroy(st->last);
    delete st;
}

static StreamState *stream_state(qpp_ctx *ctx, hipStream_t s) {
    for (StreamState *st : ctx->streams)
        if (st->stream == s) return st;
    StreamState *st = new StreamState();
    st->stream = s;
    if (hipEventCreateWithFlags(&st->last, hipEventDisableTiming) != hipSuccess) {
        delete st;
        return nullptr;
    }
    ctx->streams.push_back(st);
    return st;
}

// Before enqueueing a batch on st: its launches must see every key installed so far (device-side wait).
static int see_keys(qpp_ctx *ctx, StreamState *st) {
    if (st->key_gen == ctx->key_gen) return QPP_OK;
    HIP_TRY(ctx, hipStreamWaitEvent(st->stream, ctx->keys_ready, 0));
    st->key_gen = ctx->key_gen;
    return QPP_OK;
}

int note_work(qpp_ctx *ctx, StreamState *st) {
    HIP_TRY(ctx, hipEventRecord(st->last, st->stream));
    st->used = true;
    return QPP_OK;
}

int batch_stream(qpp_ctx *ctx, void *stream, StreamState **out) {
    StreamState *st = stream_state(ctx, stream ? (hipStream_t)stream : ctx->stream);
    if (!st) return QPP_DEVICE_ERROR;
    RC_TRY(see_keys(ctx, st));
    *out = st;
    return QPP_OK;
}

}  // namespace qpp

extern "C" {

int qpp_abi_version(void) { return QPP_ABI_VERSION; }

int qpp_ctx_create(int device, qpp_ctx **out) {
    if (!out) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return QPP_DEVICE_ERROR;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return QPP_DEVICE_ERROR;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QPP_DEVICE_ERROR;  // kernels are built for gfx950 only
    qpp_ctx *ctx = new qpp_ctx();
    ctx->device = device;
    ctx->n_cu = (uint32_t)prop.multiProcessorCount;
    if (const char *e = getenv("QPP_BURST_MAX")) ctx->burst_max = (uint32_t)strtoul(e, nullptr, 10);
    if (const char *e = getenv("QPP_PACKET_SERVER")) ctx->pkt_server = strcmp(e, "0") != 0;
    if (const char *e = getenv("QPP_AES_KERNEL"))
        ctx->aes_kernel = !strcmp(e, "quad") || !strcmp(e, "lane") ? QPP_AES_KERNEL_QUAD
                        : !strcmp(e, "wave")                     ? QPP_AES_KERNEL_WAVE
                                                                 : 0;
    int rc = QPP_OK;
    do {
        if (fail(ctx, hipSetDevice(device), "hipSetDevice")) { rc = QPP_DEVICE_ERROR; break; }
        if (fail(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "stream") ||
            fail(ctx, hipStreamCreateWithFlags(&ctx->kstream, hipStreamNonBlocking), "key stream") ||
            fail(ctx, hipStreamCreateWithFlags(&ctx->rstream, hipStreamNonBlocking), "retire stream") ||
            fail(ctx, hipEventCreateWithFlags(&ctx->keys_ready, hipEventDisableTiming), "key event")) {
            rc = QPP_DEVICE_ERROR;
            break;
        }
        if (!stream_state(ctx, ctx->stream)) { rc = QPP_DEVICE_ERROR; break; }
        if (fail(ctx, dmalloc(ctx, &ctx->d_diag, 64), "diag") ||
            fail(ctx, hipMemsetAsync(ctx->d_diag, 0, 64, ctx->stream), "diag") ||
            fail(ctx, hipStreamSynchronize(ctx->stream), "diag")) {
            rc = QPP_DEVICE_ERROR;
            break;
        }
        rc = grow_keys(ctx, 64);
    } while (0);
    if (rc) {
        qpp_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return QPP_OK;
}

int qpp_ctx_set_aes_kernel(qpp_ctx *ctx, int kernel) {
    if (!ctx || kernel < QPP_AES_KERNEL_AUTO || kernel > QPP_AES_KERNEL_WAVE) return QPP_INTERNAL_ERROR;
    ctx->aes_kernel = kernel;
    return QPP_OK;
}

int qpp_ctx_set_fips(qpp_ctx *ctx, int on) {
    if (!ctx) return QPP_INTERNAL_ERROR;
    ctx->fips = on != 0;
    return QPP_OK;
}

int qpp_ctx_set_burst_max(qpp_ctx *ctx, size_t max_packets) {
    if (!ctx) return QPP_INTERNAL_ERROR;
    ctx->burst_max = max_packets > UINT32_MAX ? UINT32_MAX : (uint32_t)max_packets;
    return QPP_OK;
}

void qpp_ctx_destroy(qpp_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    qpp_txq_destroy(ctx->pkt_q);
    ctx->pkt_q = nullptr;
    if (ctx->d_keys) flush_retire(ctx);  // pending zeroizations, while the table and the stream states still exist
    servers_stop(ctx);
    ctx_sync(ctx);  // (the context's streams only: another context's resident servers may run on)
    dfree_zeroed(ctx, ctx->d_keys, sizeof(DevKey) * ctx->key_cap);
    secure_zero(ctx->h_keys.data(), sizeof(DevKey) * ctx->h_keys.size());
    dfree_zeroed(ctx, ctx->pow.base, (size_t)ctx->pow.cap * kPowBytes);
    for (StreamState *st : ctx->streams) free_stream_state(ctx, st);
    ctx->streams.clear();
    for (Retired &r : ctx->retired) hipEventDestroy(r.done);
    for (hipEvent_t e : ctx->event_pool) hipEventDestroy(e);
    if (ctx->pipe) {
        pipe_release(ctx);
        for (auto &t : ctx->pipe->tickets) hipEventDestroy(t.second);
        if (ctx->pipe->h2d) hipStreamDestroy(ctx->pipe->h2d);
        if (ctx->pipe->comp) hipStreamDestroy(ctx->pipe->comp);
        if (ctx->pipe->d2h) hipStreamDestroy(ctx->pipe->d2h);
        delete ctx->pipe;
    }
    dfree(ctx, ctx->d_stage);
    dfree(ctx, ctx->d_connmap);
    dfree(ctx, ctx->d_diag);
    hfree(ctx, ctx->h_connstage);
    if (ctx->connstage_ev) hipEventDestroy(ctx->connstage_ev);
    hfree(ctx, ctx->h_stage);
    for (KStage &k : ctx->kstage) {
        dfree(ctx, k.d);
        if (k.h) { secure_zero(k.h, k.cap); hfree(ctx, k.h); }
        if (k.free_ev) hipEventDestroy(k.free_ev);
    }
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->kstream) hipStreamDestroy(ctx->kstream);
    if (ctx->rstream) hipStreamDestroy(ctx->rstream);
    if (ctx->keys_ready) hipEventDestroy(ctx->keys_ready);
    if (ctx->fips_order) hipEventDestroy(ctx->fips_order);
    delete ctx;
}

void *qpp_ctx_stream(qpp_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int qpp_ctx_synchronize(qpp_ctx *ctx) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_retire(ctx));
    RC_TRY(servers_stop(ctx));  // (restarted by the next flush of their queue)
    RC_TRY(ctx_sync(ctx));      // every stream of the context (not the device: other contexts' servers run on)
    hfree(ctx, nullptr);        // pinned buffers parked while other contexts' servers were resident
    return QPP_OK;
}

const char *qpp_ctx_last_error(qpp_ctx *ctx) { return ctx ? ctx->last_error.c_str() : "no context"; }

int qpp_ctx_rx_timeouts(qpp_ctx *ctx, uint64_t *count) {
    if (!ctx || !count) return QPP_INTERNAL_ERROR;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (StreamState *st : ctx->streams) HIP_TRY(ctx, hipStreamSynchronize(st->stream));
    uint32_t v = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&v, ctx->d_diag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = v;
    return QPP_OK;
}

// ---------------------------------------------------------------- plumbing

int qpp_dev_alloc(qpp_ctx *ctx, size_t bytes, void **out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dmalloc(ctx, out, bytes));
    return QPP_OK;
}
void qpp_dev_free(qpp_ctx *ctx, void *ptr) {
    if (!ptr) return;
    hipSetDevice(ctx->device);
    dfree(ctx, ptr);  // behind the work every stream of the context has been given so far
}
int qpp_host_alloc(qpp_ctx *ctx, size_t bytes, void **out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hmalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return QPP_OK;
}
void qpp_host_free(qpp_ctx *ctx, void *ptr) {
    if (!ptr) return;
    if (!ctx) {
        hipHostFree(ptr);
        return;
    }
    hfree(ctx, ptr);  // (parked while a server of the device is resident)
}
int qpp_memcpy_d2d(qpp_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, user_stream(ctx, stream)));
    return QPP_OK;
}

int qpp_memcpy_h2d(qpp_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, user_stream(ctx, stream)));
    return QPP_OK;
}
int qpp_memcpy_d2h(qpp_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, user_stream(ctx, stream)));
    return QPP_OK;
}
int qpp_memset_d(qpp_ctx *ctx, void *dst, int value, size_t bytes, void *stream) {
    HIP_TRY(ctx, hipMemsetAsync(dst, value, bytes, user_stream(ctx, stream)));
    return QPP_OK;
}
int qpp_stream_create(qpp_ctx *ctx, void **out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    user_stream(ctx, (void *)s);
    *out = (void *)s;
    return QPP_OK;
}
void qpp_stream_destroy(qpp_ctx *ctx, void *stream) {
    if (!stream) return;
    hipStream_t s = (hipStream_t)stream;
    if (ctx && s != ctx->stream) {
        hipStreamSynchronize(s);  // its batches are done: its plan scratch and last-batch event can go
        for (size_t i = 0; i < ctx->streams.size(); i++) {
            StreamState *st = ctx->streams[i];
            if (st->stream != s) continue;
            free_stream_state(ctx, st);
            ctx->streams.erase(ctx->streams.begin() + (long)i);
            break;
        }
        ctx->user_streams.erase(std::remove(ctx->user_streams.begin(), ctx->user_streams.end(), s),
                                ctx->user_streams.end());
    }
    hipStreamDestroy(s);
}
int qpp_stream_synchronize(qpp_ctx *ctx, void *stream) {
    HIP_TRY(ctx, hipStreamSynchronize(stream ? (hipStream_t)stream : ctx->stream));
    return QPP_OK;
}
int qpp_event_create(qpp_ctx *ctx, void **out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t e;
    HIP_TRY(ctx, hipEventCreate(&e));
    *out = (void *)e;
    return QPP_OK;
}
void qpp_event_destroy(qpp_ctx *, void *event) {
    if (event) hipEventDestroy((hipEvent_t)event);
}
int qpp_event_record(qpp_ctx *ctx, void *event, void *stream) {
    HIP_TRY(ctx, hipEventRecord((hipEvent_t)event, user_stream(ctx, stream)));
    return QPP_OK;
}
int qpp_event_elapsed_ms(qpp_ctx *ctx, void *start, void *stop, float *ms) {
    HIP_TRY(ctx, hipEventSynchronize((hipEvent_t)stop));
    HIP_TRY(ctx, hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return QPP_OK;
}

int qpp_stream_wait_event(qpp_ctx *ctx, void *stream, void *event) {
    HIP_TRY(ctx, hipStreamWaitEvent(user_stream(ctx, stream), (hipEvent_t)event, 0));
    return QPP_OK;
}

}  // extern "C"
