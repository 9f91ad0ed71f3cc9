// servers.cpp -- the resident server kernels of a device: the process-wide registry, the park-or-evict allocator on
// top of it, and the life of one queue's server (start, wait, one-shot finish, stop).
#include "host.h"

namespace qpp {

// ---------------------------------------------------------------- resident servers of a device (process-wide)
// Persistent server kernels -- transmit-queue servers and the contexts' packet servers -- hold whole CUs while they run,
// and their streams share the device's greatest-priority hardware queues.  One registry per device, over every context
// of the process:
//   * cu_avail counts the workgroups of EVERY resident server of the device, so a full-chip grid -- above all the fused
//     receive's, whose grid barriers need every workgroup resident at once -- is sized for the CUs really left;
//   * fused receives of the device run one after another (each waits, device side, for the previous one: two on two
//     streams would split the CUs and both time out), and a server launch waits for the latest fused receive (a server
//     starting while a receive's workgroups are being dispatched would take CUs the receive's grid counted on);
//   * at most GPU_MAX_HW_QUEUES (default 4) servers are resident per device: the runtime maps the streams of one
//     priority level onto that many hardware queues, and a server launched onto a hardware queue a resident server
//     holds would wait for that server's idle exit.  A queue finding no free server slot takes the launched path (a
//     transmit-queue flush) or launches the per-packet kernel (the packet server's callers).
DevServers &dev_servers(int device) {
    static DevServers regs[64];
    return regs[(unsigned)device & 63u];
}
// past this many parked bytes per device, release evicts the device's resident servers and frees; env QPP_PARKED_MAX_MB
static size_t parked_max() {
    static const size_t v = [] {
        const char *e = getenv("QPP_PARKED_MAX_MB");
        return e ? (size_t)strtoull(e, nullptr, 10) << 20 : size_t(2) << 30;
    }();
    return v;
}
static uint32_t server_slots() {
    static const uint32_t n = [] {
        const char *e = getenv("GPU_MAX_HW_QUEUES");
        const unsigned long v = e ? strtoul(e, nullptr, 10) : 4ul;
        return (uint32_t)(v ? std::min(v, 32ul) : 4ul);
    }();
    return n;
}
// launched and its stream still busy: read-only on the queue, safe for another context's thread (registry lock held)
static bool srv_resident(const qpp_txq *q) {
    return q->srv_launched.load(std::memory_order_acquire) && hipStreamQuery(q->srv_stream) == hipErrorNotReady;
}
uint32_t resident_wgs_locked(const DevServers &r) {
    uint32_t w = 0;
    for (const qpp_txq *o : r.queues)
        if (srv_resident(o)) w += o->srv_wgs;
    return w;
}

// Frees p at once when no server of the device is resident, else parks it, up to parked_max() bytes per device.  Past
// that bound the device's resident servers -- every context's -- are EVICTED: the eviction word makes each leave at its
// next poll that finds no complete flush (a flush it has seen is finished first), their streams are waited for (a
// poll, or the flush in hand: microseconds), and only then does hipFree run -- it never waits for a server that keeps
// being fed.  An evicted queue's owner relaunches its server at its next post (srv_prepare),
// and a flush posted while its server left is picked up by the relaunched one (srv_wait).  p = nullptr only frees what
// is parked, if it can.  Under the registry lock throughout, so no server starts between the wait and the free.
void release(qpp_ctx *ctx, void *p, bool pinned) {
    DevServers &r = dev_servers(ctx->device);
    std::unique_lock<std::mutex> lk(r.mu);
    auto resident = [&r] {
        for (const qpp_txq *o : r.queues)
            if (srv_resident(o)) return true;
        return false;
    };
    size_t bytes = p ? take_size(p) : 0;
    if (p && !bytes) bytes = size_t(1) << 20;  // (not allocated through this library: counted as 1 MiB)
    if (resident()) {
        if (!p) return;
        if (r.parked_bytes + bytes <= parked_max()) {
            r.parked.emplace_back(p, pinned);
            r.parked_bytes += bytes;
            return;
        }
        if (r.h_evict) {
            __atomic_store_n(r.h_evict, 1u, __ATOMIC_RELEASE);
            for (qpp_txq *o : r.queues) {
                if (!o->srv_launched.load(std::memory_order_acquire)) continue;
                hipStreamSynchronize(o->srv_stream);  // (its server leaves at its next poll)
                o->evicted.store(true, std::memory_order_release);
            }
            __atomic_store_n(r.h_evict, 0u, __ATOMIC_RELEASE);
            r.evictions++;
        }
    }
    for (const auto &x : r.parked) {
        if (x.second) hipHostFree(x.first);
        else hipFree(x.first);
    }
    r.parked.clear();
    r.parked_bytes = 0;
    if (p) {
        if (pinned) hipHostFree(p);
        else hipFree(p);
    }
}

static uint32_t servers_cu(const qpp_ctx *ctx) {  // every resident server of the device, any context
    DevServers &r = dev_servers(ctx->device);
    std::lock_guard<std::mutex> lk(r.mu);
    return resident_wgs_locked(r);
}
uint32_t cu_avail(const qpp_ctx *ctx) {
    const uint32_t r = servers_cu(ctx);
    return ctx->n_cu > r ? ctx->n_cu - r : 1u;
}

// Launches the server unless it runs.  A flush posted but not done (posted while the last server was leaving on its
// idle timeout) is picked up by the new one: it starts with seq0 != the posted seq.
int srv_start(qpp_txq *q, bool force) {
    // (no stream query while the server is believed running: a server that left on its idle timeout is found by
    // srv_wait's slow path, which relaunches it behind the posted flush)
    if (q->srv_running && q->evicted.exchange(false, std::memory_order_acq_rel)) srv_alive(q);  // (it left)
    if (q->srv_running) return QPP_OK;
    qpp_ctx *ctx = q->ctx;
    DevServers &r = dev_servers(ctx->device);
    std::lock_guard<std::mutex> lk(r.mu);
    if (!force) {
        uint32_t n = 0;
        for (const qpp_txq *o : r.queues)
            if (o != q && srv_resident(o)) n++;
        if (n >= server_slots()) return kNoServerSlot;
    }
    // behind the device's latest fused receive (its grid did not count this server's CUs)
    if (r.rx_tail) HIP_TRY(ctx, hipStreamWaitEvent(q->srv_stream, r.rx_tail, 0));
    const bool pending = q->srv_posted && !srv_done(q, q->srv_posted);
    const uint32_t seq0 = pending ? q->srv_posted - 1u : q->srv_seq;
    HIP_TRY(ctx, launch_txq_server(ctx->d_keys, ctx->pow, q->v_mail, q->v_slots, q->v_items, q->v_sdesc, q->v_ring,
                                   (uint32_t)std::min<size_t>(q->ring_bytes, UINT32_MAX), seq0, q->srv_idle_ticks,
                                   q->srv_wgs, r.v_evict, q->srv_stream));
    q->srv_running = true;
    q->srv_launched.store(true, std::memory_order_release);
    q->srv_keys = ctx->d_keys;
    q->srv_last_post = std::chrono::steady_clock::now();  // (its idle clock starts now)
    q->n_starts++;
    return QPP_OK;
}

// A posted flush whose server left before every workgroup saw it (idle exit, or evicted by release) while every
// server slot of the device is taken: a relaunched server could land on a hardware queue a fed server holds and wait
// for that server's exit.  So the flush is finished by a ONE-SHOT launch of the server kernel (idle 0: it
// serves the posted flush in the workgroups whose `done` does not show it yet, then leaves) on the context's own
// normal-priority stream.  At most one in flight per queue.
static int srv_oneshot(qpp_txq *q) {
    qpp_ctx *ctx = q->ctx;
    if (q->oneshot_ev && hipEventQuery(q->oneshot_ev) == hipErrorNotReady) return QPP_OK;
    if (!q->oneshot_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&q->oneshot_ev, hipEventDisableTiming));
    DevServers &r = dev_servers(ctx->device);
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.rx_tail) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, r.rx_tail, 0));
    HIP_TRY(ctx, launch_txq_server(ctx->d_keys, ctx->pow, q->v_mail, q->v_slots, q->v_items, q->v_sdesc, q->v_ring,
                                   (uint32_t)std::min<size_t>(q->ring_bytes, UINT32_MAX), q->srv_posted - 1u, 0u,
                                   q->srv_wgs, r.v_evict, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(q->oneshot_ev, ctx->stream));
    q->n_starts++;
    q->n_oneshots++;
    r.oneshots++;
    return QPP_OK;
}

int srv_wait(qpp_txq *q, uint32_t seq) {
    if (!seq) return QPP_OK;
    std::chrono::steady_clock::time_point t0{};
    for (uint64_t spin = 0;; spin++) {
        if (srv_done(q, seq)) return QPP_OK;
        if ((spin & 4095u) == 4095u) {
            // it left (idle, evicted) before this flush was seen: a new one takes it -- unless a one-shot launch is
            // still on it (two kernels must never serve one flush: the ring is sealed in place)
            const bool oneshot = q->oneshot_ev && hipEventQuery(q->oneshot_ev) == hipErrorNotReady;
            if (!oneshot && !srv_alive(q)) {
                int rc = srv_start(q);
                if (rc == kNoServerSlot) rc = srv_oneshot(q);
                RC_TRY(rc);
            }
            const auto now = std::chrono::steady_clock::now();
            if (spin == 4095u) t0 = now;
            else if (now - t0 > std::chrono::seconds(10)) {
                q->ctx->last_error = "txq server: flush not completed within 10 s";
                return QPP_DEVICE_ERROR;
            }
        }
        __builtin_ia32_pause();
    }
}

int srv_stop(qpp_txq *q) {
    if (!q->srv_running) return QPP_OK;
    RC_TRY(srv_wait(q, q->srv_posted));
    if (!srv_alive(q)) return QPP_OK;
    q->srv_seq = srv_next(q->srv_seq);
    for (uint32_t b = 0; b < q->srv_wgs; b++) {
        q->h_slots[b].word = kTxsStop;
        __atomic_store_n(&q->h_slots[b].seq, q->srv_seq, __ATOMIC_RELEASE);
    }
    HIP_TRY(q->ctx, hipStreamSynchronize(q->srv_stream));
    q->srv_running = false;
    q->srv_launched.store(false, std::memory_order_release);
    return QPP_OK;
}

int srv_prepare(qpp_txq *q, std::chrono::steady_clock::time_point now) {
    qpp_ctx *ctx = q->ctx;
    RC_TRY(srv_wait(q, q->srv_posted));
    if (ctx->key_gen != q->srv_key_gen) {
        // records installed since the last post are in HBM before the server reads them (host wait, only after key
        // changes), and the new epoch drops every workgroup's cached GHASH tables (a slot may hold a new key now)
        HIP_TRY(ctx, hipEventSynchronize(ctx->keys_ready));
        q->srv_key_gen = ctx->key_gen;
        q->srv_epoch = (q->srv_epoch + 1u) & 0xffu;
    }
    // a one-shot launch that served the last flush has left before anything is posted again (it would serve it too)
    if (q->oneshot_ev) HIP_TRY(ctx, hipEventSynchronize(q->oneshot_ev));
    if (q->srv_running && q->srv_keys != ctx->d_keys) RC_TRY(srv_stop(q));  // (grow_keys stops servers already)
    // a server idle for long may be leaving on its own timeout: never post to it (part of it could miss the flush)
    if (q->srv_running && now - q->srv_last_post > q->srv_host_idle) RC_TRY(srv_stop(q));
    return QPP_OK;
}

int servers_stop(qpp_ctx *ctx) {
    for (qpp_txq *q : ctx->servers) RC_TRY(srv_stop(q));
    return QPP_OK;
}
int servers_quiesce(qpp_ctx *ctx) {
    for (qpp_txq *q : ctx->servers) RC_TRY(srv_wait(q, q->srv_posted));
    return QPP_OK;
}

}  // namespace qpp

extern "C" {

int qpp_dev_server_evictions(int device, uint64_t *evictions, uint64_t *oneshots) {
    if (device < 0 || device >= 64) return QPP_INTERNAL_ERROR;
    DevServers &r = dev_servers(device);
    std::lock_guard<std::mutex> lk(r.mu);
    if (evictions) *evictions = r.evictions;
    if (oneshots) *oneshots = r.oneshots;
    return QPP_OK;
}

}  // extern "C"
