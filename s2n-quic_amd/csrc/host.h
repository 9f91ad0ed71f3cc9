// host.h -- internal to the host runtime behind include/qpp.h (ctx.cpp, keys.cpp, batch.cpp, packet.cpp, servers.cpp,
// txq.cpp): the state those units share and the functions that cross them, each declared once here under the unit
// that defines it; the design comments live there, with the code they describe.  No CPU fallback exists: every byte of
// payload is sealed/opened by the HIP kernels; without a gfx950 device the calls fail with QPP_DEVICE_ERROR.
#pragma once

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

#include "qpp_internal.h"

using namespace qpp;  // (the handle types below are the C ABI's, so they stay outside the namespace)

namespace qpp {

struct StreamState {
    hipStream_t stream = nullptr;
    PlanBuffers plan{};
    uint32_t plan_n_cap = 0, plan_key_cap = 0;
    hipEvent_t last = nullptr;  // after this stream's latest batch
    bool used = false;          // `last` has been recorded at least once
    uint64_t key_gen = 0;       // the latest key install this stream has waited for
    // FIPS-mode nonce-order gate scratch (fips.hip): sort keys, scans, the gated descriptor copy, rocPRIM temp
    void *fips_buf = nullptr;
    size_t fips_bytes = 0;
    uint32_t fips_n_cap = 0;
    uint32_t *fips_refused = nullptr;  // device word: packets the gate refused (txq flushes report it)
    uint32_t *rx_scratch = nullptr;    // fused receive kernel (quad.hip): barrier, per-key counts / cursors, work items
    uint32_t rx_scratch_keys = 0;      // the key_cap it is sized for
    // a mixed-suite batch's ChaCha20 kernel runs on this side stream beside the AES kernel (fork after the plan, join
    // before the batch's last event): its workgroups fill the CUs the AES kernel's last workgroups leave
    hipStream_t side = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
};

struct KStage {
    uint8_t *h = nullptr, *d = nullptr;
    size_t cap = 0;
    size_t pending = 0;          // bytes of key records / secrets in h, zeroized once the job's copy is done
    hipEvent_t free_ev = nullptr;  // recorded on the key stream after the last job that reads this stage
    bool used = false;
};

struct Retired {
    std::vector<uint32_t> slots;
    hipEvent_t done;  // the zeroing of these device records (retire stream) has completed
};
constexpr size_t kRetireFlush = 4096;  // pending retirements that force a flush from qpp_key_free itself

// One slot of the host pipeline: device buffers for one chunk in flight, and the events that order its reuse.
struct PipeSlot {
    uint8_t *arena = nullptr;  // chunk span of the arena
    qpp_pkt *descs = nullptr;
    uint8_t *masks = nullptr;
    int8_t *status = nullptr;
    hipEvent_t h2d = nullptr, comp = nullptr, d2h = nullptr;
    bool busy = false;  // d2h has been recorded (the next user waits for it)
};

struct HostPipe {
    // Buffers for chunks of up to 256 Ki packets.  Unless the geometry is set (qpp_ctx_set_host_pipe), a batch is cut
    // into ~16 chunks of 64-256 Ki packets, and at least 64 packets per live AES key (one full wave-item each): with
    // 4096 keys, 64 Ki-packet chunks ran the C5 pipeline at 76 ms/step instead of 62; with one key, 256 Ki-packet
    // chunks made a 1 Mi-packet batch 33 ms instead of 29 (pipeline fill and drain).  profiles/r02_e2e.jsonl
    size_t chunk_packets = 262144, chunk_bytes = 384u << 20, nslots = 4;
    bool auto_chunk = true;
    hipStream_t h2d = nullptr, comp = nullptr, d2h = nullptr;
    std::vector<PipeSlot> slots;
    size_t next = 0;
    uint64_t next_ticket = 1;
    std::map<uint64_t, hipEvent_t> tickets;
};

}  // namespace qpp

struct qpp_ctx {
    int device = 0;
    uint32_t n_cu = 0;  // compute units (AES work-item sizing)
    uint32_t burst_max = kBurstMaxDefault;  // AES batches up to this size take the wave-per-packet kernel
    int aes_kernel = 0;  // QPP_AES_KERNEL_*: 0 = chosen per batch (aes_path)
    hipStream_t stream = nullptr;
    hipStream_t kstream = nullptr;  // key installs / derivations
    hipStream_t rstream = nullptr;  // key retirements (zeroization behind in-flight batches)
    hipEvent_t keys_ready = nullptr;
    uint64_t key_gen = 0;           // installs so far (keys_ready marks the latest)
    // device key table + host mirror
    DevKey *d_keys = nullptr;
    uint32_t key_cap = 0;
    PowTables pow{nullptr, 0};  // burst power tables of slots < pow.cap (grown with the key table, <= kPowSlots)
    std::vector<DevKey> h_keys;
    std::vector<uint8_t> dirty_flag;
    std::vector<uint32_t> dirty;          // slots whose host record must be installed before the next launch
    std::vector<uint32_t> free_slots;     // reusable now
    std::deque<Retired> retired;          // reusable once `done` has completed
    std::vector<uint32_t> retire_pending; // freed, host copy zeroized, device zeroing not yet enqueued
    uint32_t retired_slots = 0;           // slots in `retired`
    uint32_t live_by_suite[4] = {0, 0, 0, 0};  // live packet keys per suite: which kernels a batch can need
    uint32_t hdr_live_by_suite[4] = {0, 0, 0, 0};  // live header-key-only records per suite (the fused ChaCha receive)
    uint32_t live_slot_xor = 0;                  // XOR of the live packet keys' slots: THE slot when only one is live
    bool fips = false;                           // qpp_ctx_set_fips: AES packet keys created now seal in FIPS mode
    uint32_t fips_live = 0;                      // live FIPS keys: seal batches run the nonce-order gate
    // The nonce-order state lives in the device key records and the gate reads and advances it without atomics, so
    // the gates of all streams run one after another in submission order: each gate's stream waits for this event
    // (recorded behind the previous gate, on whatever stream that ran) -- two txq flushes in flight on different
    // streams could otherwise both pass a repeated packet number, or a later flush refuse an earlier one's packets.
    hipEvent_t fips_order = nullptr;
    bool fips_order_used = false;
    uint32_t next_slot = 0;
    // per-stream state (plan scratch, last-batch event); [0] is the context stream
    std::vector<StreamState *> streams;
    // every other stream the caller handed this context or got from it (qpp_stream_create; a non-null stream of
    // qpp_memcpy_*, qpp_memset_d, qpp_event_record, qpp_stream_wait_event) until qpp_stream_destroy: qpp_ctx_synchronize
    // waits for these too (a copy-only stream has no StreamState)
    std::vector<hipStream_t> user_streams;
    std::vector<hipEvent_t> event_pool;
    // per-packet staging (pinned, zero-copy) and key staging (pinned + device)
    uint8_t *d_stage = nullptr, *h_stage = nullptr;
    uint8_t *v_stage = nullptr;  // device view of the pinned h_stage (zero-copy per-packet calls)
    size_t stage_cap = 0;
    // two pinned key stages (+ device twins), used alternately by the key-stream jobs (installs, derivations): a
    // job waits only for the previous job of ITS stage (an event), never for the key stream as a whole
    KStage kstage[2];
    int kstage_next = 0;
    HostPipe *pipe = nullptr;
    std::vector<qpp_txq *> servers;  // transmit queues with a persistent server kernel (qpp_txq_create_persistent)
    std::vector<qpp_txq *> txqs;     // every transmit queue of the context (their flush streams: ctx_streams)
    // The packet server: a persistent queue of the context's own (kPktWgs workgroups, created on the first per-packet
    // call) through which qpp_seal / qpp_open run without a kernel launch; qpp_ctx_set_packet_server, QPP_PACKET_SERVER
    qpp_txq *pkt_q = nullptr;
    bool pkt_server = true;
    uint64_t pkt_calls = 0, pkt_starts = 0;  // qpp_ctx_packet_server_info (starts of freed servers in pkt_starts)
    uint32_t *d_connmap = nullptr;    // qpp_ctx_set_conn_keys: connection -> key slot (device)
    size_t connmap_cap = 0, connmap_n = 0;
    // its pinned staging copy (the caller's array is pageable: HIP does not promise an async copy from it has read it
    // when the call returns), reused once connstage_ev shows the previous copy done
    uint32_t *h_connstage = nullptr;
    size_t connstage_cap = 0;
    hipEvent_t connstage_ev = nullptr;
    bool connstage_used = false;
    uint32_t *d_diag = nullptr;  // device counters: [0] fused-receive workgroups that left on a barrier timeout
    std::string last_error;
};

struct qpp_key {
    qpp_ctx *ctx = nullptr;
    int suite = 0;
    uint32_t slot = 0;
    bool has_secret = false;
    uint8_t secret[48] = {0};
    uint8_t key[32] = {0};
    uint8_t iv[12] = {0};
    uint8_t hp[32] = {0};
};

// HeaderKey (header_key.rs:7-63): owned independently of any packet key; its own device slot (live = 2) holds only
// the header-protection key schedule.
struct qpp_header_key {
    qpp_ctx *ctx = nullptr;
    int suite = 0;
    uint32_t slot = 0;
    uint8_t hp[32] = {0};
};

// One in-flight flush of a txq: its descriptors and (zero-copy) plan in pinned memory, the device copies for the DMA
// path, the stream it went out on and the event that ends it.
struct TxqSlot {
    qpp_pkt *h_desc = nullptr, *d_desc = nullptr, *v_desc = nullptr;
    uint32_t *h_perm = nullptr;  // pinned: perm[max_packets] | n_work | WorkItem work[max_packets + 1]
    WorkItem *h_work = nullptr;
    uint32_t *h_nwork = nullptr;
    PlanBuffers v_plan{};
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint64_t first = 0, last = 0;  // tickets (bursts) of the flush that last used this slot (0: never)
    uint32_t *h_refused = nullptr;  // pinned: packets of the flush the FIPS nonce-order gate refused
    bool busy = false;    // `done` recorded and not yet seen complete
};

struct qpp_txq {
    qpp_ctx *ctx = nullptr;
    size_t ring_bytes = 0, max_packets = 0;
    uint8_t *h_ring = nullptr, *d_ring = nullptr, *v_ring = nullptr;
    // flushes in flight: the batch being pushed fills slots[cur]; flush_async sends it and moves to the next slot
    std::vector<TxqSlot> slots;
    std::vector<hipStream_t> streams;
    size_t cur = 0;
    uint64_t next_ticket = 1;
    // bursts flushed into slots[cur] but not yet submitted (coalescing): tickets [pend_first, pend_last]
    uint64_t pend_first = 0, pend_last = 0;
    uint32_t pend_bursts = 0, coalesce = 1;
    size_t count = 0, lo = SIZE_MAX, hi = 0;
    size_t count_at_ticket = 0;  // q->count at the last flush_async (packets pushed since belong to the next ticket)
    uint32_t suites = 0;
    // zero-copy flush of small bursts: the kernels read and write the pinned ring, descriptors and a host-built
    // plan directly over PCIe (no DMA copies, no plan launches)
    uint32_t zc_max = 0;
    std::vector<uint32_t> order;
    std::vector<std::pair<size_t, size_t>> runs;  // DMA path: the flush's contiguous packet byte ranges
    // Persistent server (qpp_txq_create_persistent; burst.hip txq_server_kernel): flushes of AES packets are posted
    // through per-workgroup slots in pinned memory instead of launched.  One posted flush at a time: its plan (work items and
    // key-sorted descriptors, pinned) is rewritten only once `done` shows the previous one sealed.
    bool persistent = false;
    TxsMail *h_mail = nullptr, *v_mail = nullptr;
    TxsSlot *h_slots = nullptr, *v_slots = nullptr;  // one per server workgroup
    WorkItem *h_items = nullptr, *v_items = nullptr;
    qpp_pkt *h_sdesc = nullptr, *v_sdesc = nullptr;
    hipStream_t srv_stream = nullptr;
    bool srv_running = false;           // launched and not yet seen to have ended
    std::atomic<bool> srv_launched{false};  // the same, readable by other contexts' threads (device registry)
    std::atomic<bool> evicted{false};       // release() made the server leave (another thread): srv_running is stale
    const DevKey *srv_keys = nullptr;   // the key table the running server reads
    uint32_t srv_seq = 0;               // seq of the last flush or stop written into the slots
    uint32_t srv_posted = 0;            // seq of the last flush posted (0: none)
    uint64_t srv_first = 0, srv_last = 0;  // its tickets
    uint32_t srv_epoch = 0;             // key epoch posted with the flushes (8 bits)
    uint64_t srv_key_gen = ~0ull;       // ctx->key_gen the server's epoch stands for
    uint32_t srv_wgs = 16, srv_idle_ticks = 0;
    std::chrono::steady_clock::time_point srv_last_post{};  // the server may leave idle_ticks after it
    std::chrono::microseconds srv_host_idle{0};             // a quarter of that: past it, restart before posting
    uint64_t n_server = 0, n_launch = 0, n_starts = 0;  // flushes posted / launched; server launches
    uint64_t n_oneshots = 0;            // of which one-shot launches finishing a posted flush (srv_oneshot)
    hipEvent_t oneshot_ev = nullptr;    // behind the latest one
};

namespace qpp {

// The resident servers of one device, over every context of the process (servers.cpp)
struct DevServers {
    std::mutex mu;
    std::vector<qpp_txq *> queues;  // the persistent queues of every context on the device
    hipEvent_t rx_tail = nullptr;   // recorded behind the device's latest fused receive
    std::vector<std::pair<void *, bool>> parked;  // buffers (pinned: true) freed once no server is resident (release)
    size_t parked_bytes = 0;
    // the device's eviction word (16 B, coherent pinned memory; host view / device view): non-zero makes every resident
    // server of the device leave at its next poll without a complete flush (release past the parked bound)
    uint32_t *h_evict = nullptr, *v_evict = nullptr;
    uint64_t evictions = 0, oneshots = 0;  // qpp_dev_server_evictions
};

inline bool fail(qpp_ctx *ctx, hipError_t e, const char *what) {
    if (e == hipSuccess) return false;
    if (ctx) ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return true;
}
#define HIP_TRY(ctx, expr)                                      \
    do {                                                        \
        if (fail((ctx), (expr), #expr)) return QPP_DEVICE_ERROR; \
    } while (0)
#define RC_TRY(expr)          \
    do {                      \
        int rc_ = (expr);     \
        if (rc_) return rc_;  \
    } while (0)

constexpr int kNoServerSlot = 1000;  // (internal) srv_start: every server slot of the device is taken
constexpr uint32_t kAesSuites = (1u << QPP_SUITE_TLS_AES_128_GCM_SHA256) | (1u << QPP_SUITE_TLS_AES_256_GCM_SHA384);

inline bool valid_suite(int s) {
    return s == QPP_SUITE_TLS_AES_128_GCM_SHA256 || s == QPP_SUITE_TLS_AES_256_GCM_SHA384 ||
           s == QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256;
}
inline bool is_aes(int suite) { return suite != QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256; }
inline uint32_t suite_mask(const qpp_ctx *ctx) {
    uint32_t m = 0;
    for (int s = 1; s <= 3; s++)
        if (ctx->live_by_suite[s]) m |= 1u << s;
    return m;
}

// ---------------------------------------------------------------- ctx.cpp: memory, events, stream state
void note_size(void *p, size_t bytes);
size_t take_size(void *p);
template <class T>
hipError_t dmalloc(qpp_ctx *, T **p, size_t bytes) {
    const hipError_t e = hipMalloc((void **)p, bytes ? bytes : 1);
    if (e == hipSuccess) note_size((void *)*p, bytes ? bytes : 1);
    return e;
}
template <class T>
hipError_t hmalloc(T **p, size_t bytes, unsigned flags) {
    const hipError_t e = hipHostMalloc((void **)p, bytes ? bytes : 1, flags);
    if (e == hipSuccess) note_size((void *)*p, bytes ? bytes : 1);
    return e;
}
// a pinned allocation and its device view (what a kernel reads and writes it through, zero-copy)
template <class T, class V>
hipError_t hmalloc_mapped(T **host, V **view, size_t bytes, unsigned flags) {
    void *v = nullptr;
    hipError_t e = hmalloc(host, bytes, flags);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&v, *host, 0);
    *view = (V *)v;
    return e;
}
void hfree(qpp_ctx *ctx, void *p);
void dfree(qpp_ctx *ctx, void *p);
// zeroize on the context stream, wait, then free (key material, packet bytes); nothing else may still use p
void dfree_zeroed(qpp_ctx *ctx, void *p, size_t bytes);
hipEvent_t get_event(qpp_ctx *ctx);
void put_event(qpp_ctx *ctx, hipEvent_t e);
int ctx_sync(qpp_ctx *ctx);
// (the plan's stream has been synchronized)
void free_plan(qpp_ctx *ctx, PlanBuffers &p);
// After enqueueing a batch on st: remember where it ends (key retirement orders behind it).
int note_work(qpp_ctx *ctx, StreamState *st);
// The stream state of a batch call on `stream` (NULL: the context stream), ready for launches.
int batch_stream(qpp_ctx *ctx, void *stream, StreamState **out);

// ---------------------------------------------------------------- keys.cpp
int grow_keys(qpp_ctx *ctx, uint32_t need);
// Installs every pending host record on the device: one copy + one install launch on the key stream, then the
// keys_ready event that the next batch on every stream waits for (device side; H and V[m] included).
int flush_keys(qpp_ctx *ctx);
int flush_retire(qpp_ctx *ctx);

// ---------------------------------------------------------------- batch.cpp
// FIPS gate scratch for batches of up to n packets on st (plus its refused-packet counter)
int ensure_fips(qpp_ctx *ctx, StreamState *st, uint32_t n);
// FIPS mode: the descriptors the seal kernels read instead of descs (refused packets skipped; status / refused count
// written).  Unchanged when no FIPS key is live.
int fips_gate(qpp_ctx *ctx, StreamState *st, const qpp_pkt *&descs, uint32_t n, int8_t *status, uint32_t *refused);
// Batch bodies: plan (AES) + kernels on st's stream; keys already flushed.  An open passes masks = nullptr.
int enqueue_batch(qpp_ctx *ctx, StreamState *st, bool seal, const qpp_pkt *descs, uint32_t n, uint8_t *arena,
                  uint8_t *masks, int8_t *status, uint32_t flags, uint32_t *refused = nullptr);
void pipe_release(qpp_ctx *ctx);

// ---------------------------------------------------------------- servers.cpp
DevServers &dev_servers(int device);
uint32_t resident_wgs_locked(const DevServers &r);
void release(qpp_ctx *ctx, void *p, bool pinned);
// CUs a full-chip kernel (one workgroup per CU) should size its grid for: those of the device's resident servers --
// every context's -- are taken
uint32_t cu_avail(const qpp_ctx *ctx);

inline uint32_t srv_next(uint32_t s) { return s + 1u ? s + 1u : 1u; }  // 0 is never a flush's seq
inline bool srv_alive(qpp_txq *q) {
    if (!q->srv_running) return false;
    if (hipStreamQuery(q->srv_stream) == hipErrorNotReady) return true;
    q->srv_running = false;  // it ended on its own (idle timeout), or failed (the next launch reports that)
    q->srv_launched.store(false, std::memory_order_release);
    return false;
}
// every workgroup has sealed the flush with this seq
inline bool srv_done(const qpp_txq *q, uint32_t seq) {
    for (uint32_t b = 0; b < q->srv_wgs; b++)
        if (__atomic_load_n(&q->h_slots[b].done, __ATOMIC_ACQUIRE) != seq) return false;
    return true;
}
// One workgroup's slot of the post `seq`: its first item `it` and that item's it.count descriptors d, every 16-byte
// chunk tagged, then the seq (x86 stores are seen in order; the server reads each chunk in one load and checks every
// tag, so a read that raced these stores is repeated)
inline void srv_write_slot(TxsSlot &sl, uint32_t seq, uint32_t word, const WorkItem &it, const qpp_pkt *d) {
    sl.word = word;
    for (uint32_t k = 0; k < it.count; k++) {
        TxsSlotDesc &sd = sl.desc[k];
        sd.pn = d[k].pn;
        sd.key_idx = d[k].key_idx;
        __atomic_store_n(&sd.tag0, seq, __ATOMIC_RELEASE);  // (after the chunk's other words)
        sd.off = d[k].off;
        sd.lens = (uint32_t)d[k].aad_len | (uint32_t)d[k].pt_len << 16;
        sd.misc = (uint32_t)d[k].pn_len | (uint32_t)d[k].flags << 8;
        __atomic_store_n(&sd.tag1, seq, __ATOMIC_RELEASE);
    }
    sl.it_key = it.key;
    sl.it_count = it.count;
    sl.it_nr = it.nr;
    __atomic_store_n(&sl.it_tag, seq, __ATOMIC_RELEASE);
    __atomic_store_n(&sl.seq, seq, __ATOMIC_RELEASE);
}
// force: a posted flush waits for this server (srv_wait's restart), so it starts even past the device's server slots
int srv_start(qpp_txq *q, bool force = false);
// Host wait for the flush with this seq (spinning on the pinned `done` word: no interrupt, no runtime call).
int srv_wait(qpp_txq *q, uint32_t seq);
int srv_stop(qpp_txq *q);
// Before a post: the previous one done, key records installed since visible to the server (and a new key epoch), the
// server on the current key table and not possibly leaving on its idle timeout
int srv_prepare(qpp_txq *q, std::chrono::steady_clock::time_point now);
// A server kernel never ends on its own while flushes keep coming, so every device-wide wait first stops the context's
// (servers_stop), and key retirement first waits for their flushes in flight (servers_quiesce).
int servers_stop(qpp_ctx *ctx);
int servers_quiesce(qpp_ctx *ctx);

// ---------------------------------------------------------------- txq.cpp
// A queue with a persistent server of `wgs` workgroups (idle exit: QPP_TXQ_SERVER_IDLE_MS)
int txq_create_server(qpp_ctx *ctx, size_t ring_bytes, size_t max_packets, uint32_t wgs, qpp_txq **out);

}  // namespace qpp
