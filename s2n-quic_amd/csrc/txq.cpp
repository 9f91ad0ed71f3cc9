// txq.cpp -- the deferred transmit queue: packets pushed into a pinned ring are sealed by one flush -- zero-copy on
// the ring, through device copies, or posted to the queue's persistent server.
#include "host.h"

namespace qpp {

// ring_flags: hipHostMallocDefault (launched flushes), or coherent + mapped (a server's ring, see txq_create_server)
static int txq_create(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, size_t in_flight, unsigned ring_flags,
                      qpp_txq **out) {
    if (!ctx || !out || !ring_bytes || !max_packets || ring_bytes > UINT32_MAX || max_packets > UINT32_MAX ||
        !in_flight || in_flight > 64)
        return QPP_INTERNAL_ERROR;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    qpp_txq *q = new qpp_txq();
    q->ctx = ctx;
    q->ring_bytes = ring_bytes;
    q->max_packets = max_packets;
    auto bad = [&](hipError_t e, const char *what) {
        if (!fail(ctx, e, what)) return false;
        qpp_txq_destroy(q);
        return true;
    };
    if (bad(hmalloc_mapped(&q->h_ring, &q->v_ring, ring_bytes, ring_flags), "txq ring") ||
        bad(dmalloc(ctx, &q->d_ring, ring_bytes), "txq ring"))
        return QPP_DEVICE_ERROR;
    // one stream per in-flight flush up to 4 (the hardware queues a process gets), shared round-robin beyond
    const size_t nstreams = in_flight < 4 ? in_flight : 4;
    for (size_t i = 0; i < nstreams; i++) {
        hipStream_t st = nullptr;
        if (bad(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "txq stream")) return QPP_DEVICE_ERROR;
        q->streams.push_back(st);
    }
    q->slots.resize(in_flight);
    for (size_t i = 0; i < in_flight; i++) {
        TxqSlot &sl = q->slots[i];
        sl.stream = q->streams[i % nstreams];
        if (bad(hmalloc_mapped(&sl.h_desc, &sl.v_desc, sizeof(qpp_pkt) * max_packets, hipHostMallocDefault),
                "txq descs") ||
            bad(dmalloc(ctx, &sl.d_desc, sizeof(qpp_pkt) * max_packets), "txq descs") ||
            bad(hmalloc_mapped(&sl.h_perm, &sl.v_plan.perm,
                               4 * (max_packets + 4) + sizeof(WorkItem) * (max_packets + 1), hipHostMallocDefault),
                "txq plan") ||
            bad(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), "txq event") ||
            bad(hmalloc(&sl.h_refused, 64, hipHostMallocDefault), "txq refused count"))
            return QPP_DEVICE_ERROR;
        *sl.h_refused = 0;
        sl.h_nwork = sl.h_perm + max_packets;
        sl.h_work = (WorkItem *)(sl.h_perm + max_packets + 4);  // 16-byte aligned
        sl.v_plan.n_work = sl.v_plan.perm + max_packets;
        sl.v_plan.work = (WorkItem *)(sl.v_plan.perm + max_packets + 4);
    }
    q->zc_max = kTxqZeroCopyMax;
    if (const char *e = getenv("QPP_TXQ_ZC_MAX")) q->zc_max = (uint32_t)strtoul(e, nullptr, 10);
    q->order.reserve(max_packets);
    memset(q->h_ring, 0, ring_bytes);
    ctx->txqs.push_back(q);
    *out = q;
    return QPP_OK;
}

static uint32_t srv_idle_ms() {
    const char *e = getenv("QPP_TXQ_SERVER_IDLE_MS");
    return e ? (uint32_t)strtoul(e, nullptr, 10) : 200u;
}

// Fine-grained (coherent) pinned memory for everything the server touches: polled over PCIe while the host writes it,
// and read and written by a kernel that does not end between flushes (no cached copy may outlive a flush) -- the ring
// too.
int txq_create_server(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, uint32_t wgs, qpp_txq **out) {
    if (!ctx || !out || max_packets >= kTxsItemsMask) return QPP_INTERNAL_ERROR;
    const unsigned fl = hipHostMallocCoherent | hipHostMallocMapped;
    RC_TRY(txq_create(ctx, ring_bytes, max_packets, 1, fl, out));
    qpp_txq *q = *out;
    auto bad = [&](hipError_t e, const char *what) {
        if (!fail(ctx, e, what)) return false;
        qpp_txq_destroy(q);
        *out = nullptr;
        return true;
    };
    q->persistent = true;
    ctx->servers.push_back(q);
    hipError_t ev_err = hipSuccess;
    {
        DevServers &r = dev_servers(ctx->device);
        std::lock_guard<std::mutex> lk(r.mu);
        if (!r.h_evict) {  // (process lifetime: one 16-B word per device, never freed)
            ev_err = hmalloc_mapped(&r.h_evict, &r.v_evict, 16, fl);
            if (ev_err == hipSuccess) memset(r.h_evict, 0, 16);
            else r.h_evict = nullptr;
        }
        r.queues.push_back(q);
    }
    if (bad(ev_err, "eviction word")) return QPP_DEVICE_ERROR;
    const size_t W = kTxsWaves;
    if (bad(hmalloc_mapped(&q->h_mail, &q->v_mail, sizeof(TxsMail), fl), "txq server mailbox") ||
        bad(hmalloc_mapped(&q->h_items, &q->v_items, sizeof(WorkItem) * max_packets, fl), "txq server items") ||
        bad(hmalloc_mapped(&q->h_sdesc, &q->v_sdesc, sizeof(qpp_pkt) * max_packets * W, fl), "txq server descs"))
        return QPP_DEVICE_ERROR;
    memset(q->h_mail, 0, sizeof(TxsMail));
    memset(q->h_sdesc, 0, sizeof(qpp_pkt) * max_packets * W);
    // The server's stream at the device's greatest priority: the runtime maps streams onto at most GPU_MAX_HW_QUEUES
    // hardware queues per priority level, round-robin, and a kernel queued behind a persistent one on the same hardware
    // queue waits for its idle exit -- found by tests/test_gpu_txrx.py: after another context's streams had come and
    // gone, the context's batch stream shared the server's queue and its seal started 30 s late.  A priority level of
    // its own keeps the servers off the batch streams' queues (at most GPU_MAX_HW_QUEUES servers per process).
    int prio_least = 0, prio_greatest = 0;
    if (bad(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest), "stream priorities") ||
        bad(hipStreamCreateWithPriority(&q->srv_stream, hipStreamNonBlocking, prio_greatest), "txq server stream"))
        return QPP_DEVICE_ERROR;
    q->srv_wgs = std::max(1u, std::min(wgs, ctx->n_cu));
    if (bad(hmalloc_mapped(&q->h_slots, &q->v_slots, sizeof(TxsSlot) * q->srv_wgs, fl), "txq server slots"))
        return QPP_DEVICE_ERROR;
    memset(q->h_slots, 0, sizeof(TxsSlot) * q->srv_wgs);
    const uint32_t idle_ms = std::min<uint32_t>(std::max(4u, srv_idle_ms()), 40000u);
    q->srv_idle_ticks = idle_ms * 100000u;  // s_memrealtime: 100 MHz
    q->srv_host_idle = std::chrono::microseconds(250u * idle_ms);
    return QPP_OK;
}

// Cuts ord[] (packet indices into desc) into work items of at most `per` packets of one key, sorting it by key first
// unless `sorted`: item(slot, b, count) for ord[b, b + count).  Returns the number of keys.
template <class F>
static uint32_t key_items(const qpp_pkt *desc, std::vector<uint32_t> &ord, bool sorted, uint32_t per, F item) {
    if (!sorted)
        std::stable_sort(ord.begin(), ord.end(),
                         [desc](uint32_t a, uint32_t b) { return desc[a].key_idx < desc[b].key_idx; });
    const uint32_t n = (uint32_t)ord.size();
    uint32_t keys = 0;
    for (uint32_t i = 0, j; i < n; i = j, keys++) {
        const uint32_t slot = desc[ord[i]].key_idx;
        for (j = i; j < n && desc[ord[j]].key_idx == slot;) j++;
        for (uint32_t b = i; b < j; b += per) item(slot, b, std::min(per, j - b));
    }
    return keys;
}

// Zero-copy flush: host plan (AES packets grouped by key, work items of whole waves) in the slot's pinned memory,
// then the burst kernel (AES) and the ChaCha kernel on the pinned ring itself; one launch per suite family.
static int txq_enqueue_zero_copy(qpp_txq *q, TxqSlot &sl, StreamState *st, uint32_t n) {
    qpp_ctx *ctx = q->ctx;
    hipStream_t s = sl.stream;
    const qpp_pkt *descs = sl.v_desc;
    RC_TRY(fips_gate(ctx, st, descs, n, nullptr, st->fips_refused));
    if (q->suites & kAesSuites) {
        std::vector<uint32_t> &ord = q->order;
        ord.clear();
        for (uint32_t i = 0; i < n; i++)
            if (is_aes(ctx->h_keys[sl.h_desc[i].key_idx].suite)) ord.push_back(i);
        const uint32_t per = burst_packets_per_item((uint32_t)ord.size(), ctx->n_cu);
        uint32_t items = 0;
        const uint32_t keys = key_items(sl.h_desc, ord, false, per, [&](uint32_t slot, uint32_t b, uint32_t cnt) {
            sl.h_work[items++] = WorkItem{slot, b, cnt, ctx->h_keys[slot].nr};
        });
        std::copy(ord.begin(), ord.end(), sl.h_perm);
        *sl.h_nwork = items;
        HIP_TRY(ctx, launch_aes_gcm_burst(true, ctx->d_keys, descs, sl.v_plan, (uint32_t)ord.size(), keys, per,
                                          q->v_ring, nullptr, nullptr, QPP_HP_APPLY, q->suites & kAesSuites, ctx->pow,
                                          s));
    }
    if (q->suites & ~kAesSuites)
        HIP_TRY(ctx, launch_chacha(true, ctx->d_keys, ctx->key_cap, descs, n, q->v_ring, nullptr, nullptr,
                                   QPP_HP_APPLY, true, s));
    return QPP_OK;
}

// the slot's last flush is over (host wait); its buffers may be refilled
static int txq_slot_drain(qpp_txq *q, TxqSlot &sl) {
    if (!sl.busy) return QPP_OK;
    HIP_TRY(q->ctx, hipEventSynchronize(sl.done));
    sl.busy = false;
    return QPP_OK;
}
// A completed flush whose packets the FIPS nonce-order gate refused (left unsealed in the ring) reports
// QPP_INTERNAL_ERROR once: to the first wait / poll of one of its tickets, or else to the flush that reuses its slot.
static int txq_refused(TxqSlot &sl) {
    if (!*sl.h_refused) return QPP_OK;
    *sl.h_refused = 0;
    return QPP_INTERNAL_ERROR;
}

// The pushed batch is handed over: the next pushes start a new one
static void txq_reset_batch(qpp_txq *q) {
    q->pend_first = q->pend_last = 0;
    q->pend_bursts = 0;
    q->count = q->count_at_ticket = 0;
    q->lo = SIZE_MAX;
    q->hi = 0;
    q->suites = 0;
}

// Persistent queue: posts slots[cur]'s packets (any suite, no FIPS key live) to the server.  The descriptors are copied
// into the server's plan (key-sorted, items of <= one packet per wave), so the slot is free for the next pushes at
// once; the previous posted flush must be done first (its plan is being rewritten).
// (the caller ran srv_prepare and started the server)
static int srv_submit(qpp_txq *q, std::chrono::steady_clock::time_point now) {
    qpp_ctx *ctx = q->ctx;
    TxqSlot &sl = q->slots[q->cur];
    const uint32_t n = (uint32_t)q->count;
    const uint32_t W = kTxsWaves;
    std::vector<uint32_t> &ord = q->order;
    ord.resize(n);
    bool one_key = true;  // (the usual GSO burst: one connection's key; no sort then)
    for (uint32_t i = 0; i < n; i++) {
        ord[i] = i;
        one_key = one_key && sl.h_desc[i].key_idx == sl.h_desc[0].key_idx;
    }
    // packets per item: spread the flush over the server's workgroups, at most one packet per wave
    const uint32_t per = std::max(1u, std::min(W, (n + q->srv_wgs - 1) / q->srv_wgs));
    uint32_t items = 0;
    key_items(sl.h_desc, ord, one_key, per, [&](uint32_t slot, uint32_t b, uint32_t cnt) {
        q->h_items[items] = WorkItem{slot, items * W, cnt, ctx->h_keys[slot].nr};
        for (uint32_t k = 0; k < cnt; k++) q->h_sdesc[(size_t)items * W + k] = sl.h_desc[ord[b + k]];
        items++;
    });
    q->srv_seq = srv_next(q->srv_seq);
    const uint32_t seq = q->srv_seq, word = (q->srv_epoch << 24) | items;
    for (uint32_t b = 0; b < q->srv_wgs; b++)  // each workgroup's slot: its first item and that item's descriptors
        srv_write_slot(q->h_slots[b], seq, word, b < items ? q->h_items[b] : WorkItem{0, 0, 0, 0},
                       q->h_sdesc + (size_t)b * W);
    q->srv_last_post = now;
    q->srv_posted = q->srv_seq;
    q->srv_first = q->pend_first;
    q->srv_last = q->pend_last;
    q->n_server++;
    txq_reset_batch(q);
    return QPP_OK;
}

// Sends slots[cur] (every burst flushed into it) and moves on to the next slot, once that one's last flush is over.
static int txq_submit(qpp_txq *q) {
    if (!q->pend_bursts) return QPP_OK;
    qpp_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));
    if (q->persistent) {
        if (!ctx->fips_live) {
            const auto now = std::chrono::steady_clock::now();
            RC_TRY(srv_prepare(q, now));
            const int rc = srv_start(q);
            if (rc != kNoServerSlot) {
                RC_TRY(rc);
                return srv_submit(q, now);
            }
            // every server slot of the device is taken: this flush is launched (the same bytes)
        }
        // FIPS gating takes the launched path (its nonce-order gate), behind the posted flush
        RC_TRY(srv_wait(q, q->srv_posted));
    }
    q->n_launch++;
    TxqSlot &sl = q->slots[q->cur];
    const uint32_t n = (uint32_t)q->count;
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, sl.stream, &st));  // sees the latest key install
    const bool gate = ctx->fips_live > 0;
    if (gate) {
        RC_TRY(ensure_fips(ctx, st, n));
        HIP_TRY(ctx, hipMemsetAsync(st->fips_refused, 0, 4, sl.stream));
    }
    if (n <= q->zc_max) {
        RC_TRY(txq_enqueue_zero_copy(q, sl, st, n));
    } else {
        hipStream_t s = sl.stream;
        // Only this flush's own packet bytes travel, as runs of adjacent packets: the ring between and around them
        // belongs to the transport or to other flushes in flight (a copy of the whole [lo, hi) span would write stale
        // device bytes over them on the way back)
        std::vector<std::pair<size_t, size_t>> &runs = q->runs;
        runs.clear();
        for (uint32_t i = 0; i < n; i++) {
            const qpp_pkt &d = sl.h_desc[i];
            runs.emplace_back((size_t)d.off, (size_t)d.off + d.aad_len + d.pt_len + 16);
        }
        std::sort(runs.begin(), runs.end());
        size_t w = 0;
        for (size_t i = 1; i < runs.size(); i++) {
            if (runs[i].first <= runs[w].second) runs[w].second = std::max(runs[w].second, runs[i].second);
            else runs[++w] = runs[i];
        }
        runs.resize(w + 1);
        for (const auto &r : runs)
            HIP_TRY(ctx, hipMemcpyAsync(q->d_ring + r.first, q->h_ring + r.first, r.second - r.first,
                                        hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_desc, sl.h_desc, sizeof(qpp_pkt) * n, hipMemcpyHostToDevice, s));
        uint32_t flags = QPP_HP_APPLY;
        if (!(q->suites & ~kAesSuites)) flags |= QPP_ONLY_AES;
        else if (!(q->suites & kAesSuites)) flags |= QPP_ONLY_CHACHA;
        RC_TRY(enqueue_batch(ctx, st, true, sl.d_desc, n, q->d_ring, nullptr, nullptr, flags, st->fips_refused));
        for (const auto &r : runs)
            HIP_TRY(ctx, hipMemcpyAsync(q->h_ring + r.first, q->d_ring + r.first, r.second - r.first,
                                        hipMemcpyDeviceToHost, s));
    }
    if (gate) HIP_TRY(ctx, hipMemcpyAsync(sl.h_refused, st->fips_refused, 4, hipMemcpyDeviceToHost, sl.stream));
    RC_TRY(note_work(ctx, st));  // key retirement orders behind this flush
    HIP_TRY(ctx, hipEventRecord(sl.done, sl.stream));
    sl.busy = true;
    sl.first = q->pend_first;
    sl.last = q->pend_last;
    txq_reset_batch(q);
    // the next batch fills the next slot, once that slot's previous flush is over (back-pressure)
    q->cur = (q->cur + 1) % q->slots.size();
    RC_TRY(txq_slot_drain(q, q->slots[q->cur]));
    return txq_refused(q->slots[q->cur]);
}

// the slot holding `ticket` (submitting it first if it is still being coalesced); nullptr: long complete
static int txq_slot_of(qpp_txq *q, uint64_t ticket, TxqSlot **out) {
    *out = nullptr;
    if (!ticket) return QPP_OK;
    if (q->pend_first && ticket >= q->pend_first && ticket <= q->pend_last) RC_TRY(txq_submit(q));
    for (TxqSlot &sl : q->slots)
        if (sl.first && ticket >= sl.first && ticket <= sl.last) { *out = &sl; break; }
    return QPP_OK;
}

// a ticket of the flush last posted to the server (earlier posted ones are done: one is posted at a time)
static bool srv_ticket(const qpp_txq *q, uint64_t ticket) {
    return q->persistent && q->srv_first && ticket >= q->srv_first && ticket <= q->srv_last;
}

}  // namespace qpp

extern "C" {

int qpp_txq_create(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, qpp_txq **out) {
    return qpp_txq_create_async(ctx, ring_bytes, max_packets, 1, out);
}

int qpp_txq_create_async(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, size_t in_flight, qpp_txq **out) {
    return txq_create(ctx, ring_bytes, max_packets, in_flight, hipHostMallocDefault, out);
}

void qpp_txq_destroy(qpp_txq *q) {
    if (!q) return;
    hipSetDevice(q->ctx->device);
    {
        std::vector<qpp_txq *> &all = q->ctx->txqs;
        all.erase(std::remove(all.begin(), all.end(), q), all.end());
    }
    servers_stop(q->ctx);  // this queue's server (and the context's others: restarted by their next call)
    if (q->persistent) {
        srv_stop(q);
        std::vector<qpp_txq *> &v = q->ctx->servers;
        v.erase(std::remove(v.begin(), v.end(), q), v.end());
        {
            DevServers &r = dev_servers(q->ctx->device);
            std::lock_guard<std::mutex> lk(r.mu);
            r.queues.erase(std::remove(r.queues.begin(), r.queues.end(), q), r.queues.end());
        }
        if (q->srv_stream) { hipStreamSynchronize(q->srv_stream); hipStreamDestroy(q->srv_stream); }
        if (q->oneshot_ev) { hipEventSynchronize(q->oneshot_ev); hipEventDestroy(q->oneshot_ev); }
        hfree(q->ctx, q->h_mail);
        if (q->h_slots) { secure_zero(q->h_slots, sizeof(TxsSlot) * q->srv_wgs); hfree(q->ctx, q->h_slots); }
        hfree(q->ctx, q->h_items);
        if (q->h_sdesc) { secure_zero(q->h_sdesc, sizeof(qpp_pkt) * q->max_packets * kTxsWaves); hfree(q->ctx, q->h_sdesc); }
    }
    for (hipStream_t st : q->streams) hipStreamSynchronize(st);
    if (q->h_ring) { secure_zero(q->h_ring, q->ring_bytes); hfree(q->ctx, q->h_ring); }
    dfree_zeroed(q->ctx, q->d_ring, q->ring_bytes);
    for (TxqSlot &sl : q->slots) {
        hfree(q->ctx, sl.h_desc);
        dfree(q->ctx, sl.d_desc);  // (the queue's streams are synchronized above)
        hfree(q->ctx, sl.h_perm);
        if (sl.done) hipEventDestroy(sl.done);
        hfree(q->ctx, sl.h_refused);
    }
    for (hipStream_t st : q->streams) {
        // the stream's StreamState (plan scratch of the DMA path) goes with it
        qpp_stream_destroy(q->ctx, (void *)st);
    }
    delete q;
}

uint8_t *qpp_txq_ring(qpp_txq *q) { return q ? q->h_ring : nullptr; }
size_t qpp_txq_pending(const qpp_txq *q) { return q ? q->count - q->count_at_ticket : 0; }

int qpp_txq_push(qpp_txq *q, const qpp_key *key, uint64_t pn, size_t off, size_t header_len, size_t pn_len,
                 size_t payload_len) {
    if (!q || !key || key->ctx != q->ctx) return QPP_INTERNAL_ERROR;
    if (q->count >= q->max_packets) return QPP_INTERNAL_ERROR;  // flush first
    if (pn_len < 1 || pn_len > 4 || header_len + pn_len > 0xffff || payload_len > 0xffff) return QPP_INTERNAL_ERROR;
    const size_t end = off + header_len + pn_len + payload_len + 16;
    if (end > q->ring_bytes || end < off) return QPP_INTERNAL_ERROR;
    if (payload_len + pn_len < 4) return QPP_DECODE_ERROR;  // the sample at header_len + 4 must fit
    qpp_pkt &d = q->slots[q->cur].h_desc[q->count++];
    d = qpp_pkt{};
    d.pn = pn;
    d.key_idx = key->slot;
    d.off = (uint32_t)off;
    d.aad_len = (uint16_t)(header_len + pn_len);
    d.pt_len = (uint16_t)payload_len;
    d.pn_len = (uint8_t)pn_len;
    q->lo = std::min(q->lo, off);
    q->hi = std::max(q->hi, end);
    q->suites |= 1u << key->suite;
    return QPP_OK;
}

int qpp_txq_push_scatter(qpp_txq *q, const qpp_key *key, uint64_t pn, size_t off, size_t header_len, size_t pn_len,
                         size_t inline_len, const uint8_t *extra, size_t extra_len) {
    if (!q || (extra_len && !extra)) return QPP_INTERNAL_ERROR;
    const size_t payload_len = inline_len + extra_len;
    if (payload_len < inline_len || off > q->ring_bytes || header_len + pn_len > q->ring_bytes - off ||
        inline_len > q->ring_bytes - off - header_len - pn_len)
        return QPP_INTERNAL_ERROR;
    const size_t at = off + header_len + pn_len + inline_len;
    RC_TRY(qpp_txq_push(q, key, pn, off, header_len, pn_len, payload_len));  // every range / capacity check
    if (extra_len) memcpy(q->h_ring + at, extra, extra_len);  // the ring holds it through end + 16 (checked above)
    return QPP_OK;
}

int qpp_txq_push_descs(qpp_txq *q, const qpp_pkt *descs, size_t n) {
    if (!q || (n && !descs)) return QPP_INTERNAL_ERROR;
    if (n > q->max_packets - q->count) return QPP_INTERNAL_ERROR;  // flush first
    qpp_ctx *ctx = q->ctx;
    for (size_t i = 0; i < n; i++) {  // the checks of qpp_txq_push, all before anything is queued
        const qpp_pkt &d = descs[i];
        if (d.key_idx >= ctx->key_cap || ctx->h_keys[d.key_idx].live != 1) return QPP_INTERNAL_ERROR;
        if (d.pn_len < 1 || d.pn_len > 4 || d.aad_len < d.pn_len || d.flags) return QPP_INTERNAL_ERROR;
        const size_t end = (size_t)d.off + d.aad_len + d.pt_len + 16;
        if (end > q->ring_bytes) return QPP_INTERNAL_ERROR;
        if ((size_t)d.pt_len + d.pn_len < 4) return QPP_DECODE_ERROR;
    }
    memcpy(q->slots[q->cur].h_desc + q->count, descs, sizeof(qpp_pkt) * n);
    for (size_t i = 0; i < n; i++) {
        const qpp_pkt &d = descs[i];
        q->lo = std::min<size_t>(q->lo, d.off);
        q->hi = std::max<size_t>(q->hi, (size_t)d.off + d.aad_len + d.pt_len + 16);
        q->suites |= 1u << ctx->h_keys[d.key_idx].suite;
    }
    q->count += n;
    return QPP_OK;
}

int qpp_txq_set_coalesce(qpp_txq *q, size_t bursts) {
    if (!q || !bursts || bursts > 1024) return QPP_INTERNAL_ERROR;
    q->coalesce = (uint32_t)bursts;
    return QPP_OK;
}

int qpp_txq_flush_async(qpp_txq *q, uint64_t *ticket) {
    if (!q || !ticket) return QPP_INTERNAL_ERROR;
    *ticket = 0;
    const size_t burst = q->count - q->count_at_ticket;
    if (!burst) return QPP_OK;  // nothing pushed since the last flush: ticket 0 is always complete
    *ticket = q->next_ticket++;
    if (!q->pend_first) q->pend_first = *ticket;
    q->pend_last = *ticket;
    q->pend_bursts++;
    q->count_at_ticket = q->count;
    // send now once `coalesce` bursts are in, or when another burst of this size would not fit the slot
    if (q->pend_bursts >= q->coalesce || q->count + burst > q->max_packets) return txq_submit(q);
    return QPP_OK;
}

int qpp_txq_poll(qpp_txq *q, uint64_t ticket, int *done) {
    if (!q || !done) return QPP_INTERNAL_ERROR;
    if (ticket >= q->next_ticket) return QPP_INTERNAL_ERROR;
    TxqSlot *sl = nullptr;
    RC_TRY(txq_slot_of(q, ticket, &sl));
    if (srv_ticket(q, ticket)) {
        *done = srv_done(q, q->srv_posted);
        if (!*done && !srv_alive(q)) RC_TRY(srv_start(q));
        return QPP_OK;
    }
    if (!sl) { *done = 1; return QPP_OK; }
    if (!sl->busy) { *done = 1; return txq_refused(*sl); }
    const hipError_t e = hipEventQuery(sl->done);
    if (e == hipErrorNotReady) { *done = 0; return QPP_OK; }
    HIP_TRY(q->ctx, e);
    sl->busy = false;
    *done = 1;
    return txq_refused(*sl);
}

int qpp_txq_wait(qpp_txq *q, uint64_t ticket) {
    if (!q) return QPP_INTERNAL_ERROR;
    if (ticket >= q->next_ticket) return QPP_INTERNAL_ERROR;
    TxqSlot *sl = nullptr;
    RC_TRY(txq_slot_of(q, ticket, &sl));
    if (srv_ticket(q, ticket)) return srv_wait(q, q->srv_posted);
    if (!sl) return QPP_OK;
    RC_TRY(txq_slot_drain(q, *sl));
    return txq_refused(*sl);
}

int qpp_txq_create_persistent(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, qpp_txq **out) {
    uint32_t wgs = 16;
    if (const char *e = getenv("QPP_TXQ_SERVER_WGS")) wgs = (uint32_t)strtoul(e, nullptr, 10);
    return txq_create_server(ctx, ring_bytes, max_packets, wgs, out);
}

int qpp_txq_server_refused(const qpp_txq *q, uint64_t *count) {
    if (!q || !count || !q->persistent) return QPP_INTERNAL_ERROR;
    *count = __atomic_load_n(&q->h_mail->oob, __ATOMIC_ACQUIRE);
    return QPP_OK;
}

int qpp_txq_server_time(const qpp_txq *q, double *us) {
    if (!q || !us || !q->persistent) return QPP_INTERNAL_ERROR;
    *us = (double)(q->h_mail->t_done - q->h_mail->t_seen) / 100.0;
    return QPP_OK;
}

int qpp_txq_server_stamps(const qpp_txq *q, uint64_t out[12]) {
    if (!q || !out || !q->persistent) return QPP_INTERNAL_ERROR;
    const TxsMail &m = *q->h_mail;
    const uint64_t v[12] = {m.t_seen, m.pad0[0], m.pad0[1], m.pad0[2], m.pad0[3], m.t_done, m.pad0[4],
                            m.pad1[0], m.pad1[1], m.pad1[2], m.pad1[3], m.pad1[4]};
    memcpy(out, v, sizeof v);
    return QPP_OK;
}

int qpp_txq_info(const qpp_txq *q, uint64_t *server_flushes, uint64_t *launched_flushes, uint64_t *server_starts) {
    if (!q) return QPP_INTERNAL_ERROR;
    if (server_flushes) *server_flushes = q->n_server;
    if (launched_flushes) *launched_flushes = q->n_launch;
    if (server_starts) *server_starts = q->n_starts;
    return QPP_OK;
}

int qpp_txq_flush(qpp_txq *q) {
    uint64_t t = 0;
    RC_TRY(qpp_txq_flush_async(q, &t));
    return qpp_txq_wait(q, t);
}

}  // extern "C"
