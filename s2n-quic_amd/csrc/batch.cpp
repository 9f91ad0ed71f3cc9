// batch.cpp -- the batch entry points: which kernels an n-packet batch takes, the plan and FIPS-gate scratch of its
// stream, seal / open / fused receive / header-protection masks over device memory, and the host pipeline for packets
// that start and end in host memory.
#include "host.h"

namespace qpp {

// Which AES-GCM kernel serves an n-packet batch: the wave-per-packet burst kernel for small batches; the quad kernel
// (quad.hip: four lanes per packet, one workgroup per CU over a slice of the key-sorted packets, 8-bit GHASH tables
// rebuilt per key segment) when the batch has >= kWaveKernelPacketsPerKey packets per live AES key; else the wave-item
// kernel (aes_gcm.hip: one key per 64-packet wave, 4-bit tables).  QPP_AES_KERNEL=quad|wave forces one of the two
// throughput kernels (A/B).
enum class AesPath { burst, quad, wave };
static AesPath aes_path(const qpp_ctx *ctx, uint32_t n) {
    if (n <= ctx->burst_max) return AesPath::burst;
    if (ctx->aes_kernel) return ctx->aes_kernel == QPP_AES_KERNEL_QUAD ? AesPath::quad : AesPath::wave;
    const uint64_t aes_keys = (uint64_t)ctx->live_by_suite[QPP_SUITE_TLS_AES_128_GCM_SHA256] +
                              ctx->live_by_suite[QPP_SUITE_TLS_AES_256_GCM_SHA384];
    const uint64_t per_key = aes_keys <= kPowSlots ? kWaveKernelPacketsPerKey : kWaveKernelPacketsPerKeyNoPow;
    return (uint64_t)n < per_key * aes_keys ? AesPath::wave : AesPath::quad;
}
static uint32_t aes_per_item(const qpp_ctx *ctx, AesPath p, uint32_t n) {
    return p == AesPath::burst ? burst_packets_per_item(n, ctx->n_cu)
           : p == AesPath::wave ? kWavePacketsPerItem
                                : kQuadPerItem;
}
static hipError_t launch_aes(const qpp_ctx *ctx, AesPath p, bool seal, const qpp_pkt *descs, const PlanBuffers &pb,
                             uint32_t n, uint8_t *arena, uint8_t *masks, int8_t *status, uint32_t flags,
                             hipStream_t s) {
    const uint32_t per = aes_per_item(ctx, p, n);
    switch (p) {
        case AesPath::burst:
            return launch_aes_gcm_burst(seal, ctx->d_keys, descs, pb, n, ctx->key_cap, per, arena, masks, status, flags,
                                        suite_mask(ctx), ctx->pow, s);
        case AesPath::wave:
            return launch_aes_gcm_wave(seal, ctx->d_keys, descs, pb, n, ctx->key_cap, cu_avail(ctx), arena, masks, status,
                                       flags, suite_mask(ctx), s);
        default:
            return launch_aes_gcm(seal, ctx->d_keys, descs, pb, n, cu_avail(ctx), arena, masks, status, flags,
                                  suite_mask(ctx), ctx->pow, s);
    }
}

// The one live packet key of the context when there is exactly one and it is an AES key: then a lane-kernel batch
// needs no plan (every AES packet is that key's; any other slot is refused in the kernel), saving the three plan
// launches (~25 us per 1 Mi batch).
static uint32_t single_aes_slot(const qpp_ctx *ctx) {
    const uint32_t live = ctx->live_by_suite[1] + ctx->live_by_suite[2] + ctx->live_by_suite[3];
    if (live != 1 || ctx->live_by_suite[QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256]) return UINT32_MAX;
    const uint32_t slot = ctx->live_slot_xor;
    return slot < ctx->key_cap && ctx->h_keys[slot].live == 1 ? slot : UINT32_MAX;
}

// The ChaCha20 kernel of a batch: after a plan that listed the non-AES packets (ChaCha20 keys, refused slots) it visits
// only those (selection mode) -- on the stream's side stream when ChaCha20 keys are live (a mixed-suite batch: it runs
// beside the AES kernel, forked behind the plan, joined before the batch ends); otherwise every packet (AES ones are
// skipped by each lane).  fork: recorded on st->stream right after the plan (the AES kernel follows it there).
static hipError_t launch_chacha_batch(const qpp_ctx *ctx, StreamState *st, bool seal, bool planned, bool forked,
                                      const qpp_pkt *descs, uint32_t n, uint8_t *arena, uint8_t *masks,
                                      int8_t *status, uint32_t flags) {
    const bool burst = n <= (ctx->burst_max >> kChachaBurstShift);
    if (planned && !burst && plan_lists_others(n, ctx->key_cap)) {
        hipStream_t s = forked ? st->side : st->stream;
        hipError_t e = launch_chacha_sel_batch(seal, ctx->d_keys, ctx->key_cap, descs, n, arena, masks, status, flags,
                                               st->plan.perm, st->plan.n_work + 4, s);
        if (e != hipSuccess || !forked) return e;
        e = hipEventRecord(st->join_ev, st->side);
        return e != hipSuccess ? e : hipStreamWaitEvent(st->stream, st->join_ev, 0);
    }
    return launch_chacha(seal, ctx->d_keys, ctx->key_cap, descs, n, arena, masks, status, flags, burst, st->stream);
}

// Whether a planned batch forks its ChaCha20 kernel onto the side stream (ChaCha20 keys live beside AES ones, a plan
// that lists them, the lane kernel): creates the side stream on first use and records the fork point
static int chacha_fork(qpp_ctx *ctx, StreamState *st, uint32_t n, uint32_t flags, bool *forked) {
    *forked = false;
    if ((flags & QPP_ONLY_AES) || !ctx->live_by_suite[QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256]) return QPP_OK;
    if (n <= (ctx->burst_max >> kChachaBurstShift) || !plan_lists_others(n, ctx->key_cap)) return QPP_OK;
    static const bool off = [] {
        const char *e = getenv("QPP_CHACHA_SIDE");
        return e && e[0] == '0';
    }();
    if (off) return QPP_OK;
    if (!st->side) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&st->side, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&st->fork_ev, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&st->join_ev, hipEventDisableTiming));
    }
    HIP_TRY(ctx, hipEventRecord(st->fork_ev, st->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(st->side, st->fork_ev, 0));
    *forked = true;
    return QPP_OK;
}

static int ensure_plan(qpp_ctx *ctx, StreamState *st, uint32_t n) {
    if (n <= st->plan_n_cap && ctx->key_cap <= st->plan_key_cap) return QPP_OK;
    HIP_TRY(ctx, hipStreamSynchronize(st->stream));  // the old scratch is no longer read
    PlanBuffers &p = st->plan;
    free_plan(ctx, p);
    st->plan_n_cap = st->plan_key_cap = 0;
    const uint32_t ncap = n, kcap = ctx->key_cap;
    HIP_TRY(ctx, dmalloc(ctx, &p.counts, sizeof(uint32_t) * kcap));
    // zeroed on the batch's own stream: plan_hist on this stream follows it.  (A plain hipMemset goes to the null
    // stream, which does not order against non-blocking streams: with recycled device memory plan_hist then counted
    // on top of stale words and the scatter wrote past perm[] -- an illegal address under two concurrent streams.)
    HIP_TRY(ctx, hipMemsetAsync(p.counts, 0, sizeof(uint32_t) * kcap, st->stream));  // plan_scan re-zeroes it after each plan
    HIP_TRY(ctx, dmalloc(ctx, &p.cursor, sizeof(uint32_t) * kcap));
    HIP_TRY(ctx, dmalloc(ctx, &p.istart, sizeof(uint32_t) * 2 * (kcap + 1)));
    HIP_TRY(ctx, dmalloc(ctx, &p.perm, sizeof(uint32_t) * std::max<uint32_t>(ncap, 1)));
    HIP_TRY(ctx, dmalloc(ctx, &p.kq, sizeof(uint32_t) * std::max<uint32_t>(ncap, 1)));
    HIP_TRY(ctx, dmalloc(ctx, &p.work, sizeof(WorkItem) * (plan_max_work(ncap, kcap, kMinPacketsPerItem) + 1)));
    HIP_TRY(ctx, dmalloc(ctx, &p.n_work, 8 * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemsetAsync(p.n_work, 0, 8 * sizeof(uint32_t), st->stream));  // (meta[6] is a running count)
    st->plan_n_cap = ncap;
    st->plan_key_cap = kcap;
    return QPP_OK;
}

// Replaces the device scratch *p by one of `bytes` once stream s, the only one that reads it, has run dry.  *cap is zero
// while *p is null: a failed allocation leaves both so, and the next call allocates again.
template <class T, class C>
static int regrow(qpp_ctx *ctx, hipStream_t s, T **p, C *cap, size_t bytes, C new_cap) {
    HIP_TRY(ctx, hipStreamSynchronize(s));  // the old scratch is no longer read
    dfree(ctx, *p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(ctx, dmalloc(ctx, p, bytes));
    *cap = new_cap;
    return QPP_OK;
}

int ensure_fips(qpp_ctx *ctx, StreamState *st, uint32_t n) {
    if (!st->fips_refused) {
        HIP_TRY(ctx, dmalloc(ctx, &st->fips_refused, 256));
        HIP_TRY(ctx, hipMemsetAsync(st->fips_refused, 0, 4, st->stream));
    }
    if (n <= st->fips_n_cap) return QPP_OK;
    const uint32_t cap = std::max<uint32_t>(n, 1024);
    st->fips_bytes = fips_scratch_bytes(cap);
    return regrow(ctx, st->stream, &st->fips_buf, &st->fips_n_cap, st->fips_bytes, cap);
}

int fips_gate(qpp_ctx *ctx, StreamState *st, const qpp_pkt *&descs, uint32_t n, int8_t *status, uint32_t *refused) {
    if (!ctx->fips_live || !n) return QPP_OK;
    RC_TRY(ensure_fips(ctx, st, n));
    if (!ctx->fips_order) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fips_order, hipEventDisableTiming));
    if (ctx->fips_order_used) HIP_TRY(ctx, hipStreamWaitEvent(st->stream, ctx->fips_order, 0));
    qpp_pkt *gated = nullptr;
    HIP_TRY(ctx, launch_fips_gate(ctx->d_keys, ctx->key_cap, descs, n, st->fips_buf, st->fips_bytes, &gated, status,
                                  refused, st->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->fips_order, st->stream));
    ctx->fips_order_used = true;
    descs = gated;
    return QPP_OK;
}

int enqueue_batch(qpp_ctx *ctx, StreamState *st, bool seal, const qpp_pkt *descs, uint32_t n, uint8_t *arena,
                  uint8_t *masks, int8_t *status, uint32_t flags, uint32_t *refused) {
    hipStream_t s = st->stream;
    bool planned = false, forked = false;
    // an open's flags choose its kernels (QPP_ONLY_*) and the fork; the kernels themselves get none, and no gate runs
    const uint32_t kflags = seal ? flags : 0;
    if (seal && !(flags & QPP_ONLY_CHACHA)) RC_TRY(fips_gate(ctx, st, descs, n, status, refused));
    if (!(flags & QPP_ONLY_CHACHA) && (suite_mask(ctx) & kAesSuites)) {
        const AesPath path = aes_path(ctx, n);
        const uint32_t one = path == AesPath::quad ? single_aes_slot(ctx) : UINT32_MAX;
        if (one != UINT32_MAX) {
            HIP_TRY(ctx, launch_aes_gcm_single(seal, ctx->d_keys, descs, one, ctx->h_keys[one].nr, n, cu_avail(ctx), arena,
                                               masks, status, kflags, ctx->pow, s));
        } else {
            RC_TRY(ensure_plan(ctx, st, n));
            HIP_TRY(ctx, launch_plan(ctx->d_keys, ctx->key_cap, descs, n, st->plan, aes_per_item(ctx, path, n), s));
            RC_TRY(chacha_fork(ctx, st, n, flags, &forked));
            HIP_TRY(ctx, launch_aes(ctx, path, seal, descs, st->plan, n, arena, masks, status, kflags, s));
            planned = true;
        }
    }
    if (!(flags & QPP_ONLY_AES))
        HIP_TRY(ctx, launch_chacha_batch(ctx, st, seal, planned, forked, descs, n, arena, masks, status, kflags));
    return QPP_OK;
}

// ---------------------------------------------------------------- host pipeline

static int pipe_init(qpp_ctx *ctx) {
    HostPipe *p = ctx->pipe;
    if (!p->h2d) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->h2d, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->comp, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->d2h, hipStreamNonBlocking));
    }
    if (p->slots.size() == p->nslots && !p->slots.empty() && p->slots[0].arena) return QPP_OK;
    p->slots.resize(p->nslots);
    for (PipeSlot &sl : p->slots) {
        HIP_TRY(ctx, dmalloc(ctx, &sl.arena, p->chunk_bytes));
        HIP_TRY(ctx, dmalloc(ctx, &sl.descs, sizeof(qpp_pkt) * p->chunk_packets));
        HIP_TRY(ctx, dmalloc(ctx, &sl.masks, 5 * p->chunk_packets));
        HIP_TRY(ctx, dmalloc(ctx, &sl.status, p->chunk_packets));
        HIP_TRY(ctx, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&sl.comp, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&sl.d2h, hipEventDisableTiming));
        sl.busy = false;
    }
    p->next = 0;
    return QPP_OK;
}

void pipe_release(qpp_ctx *ctx) {
    HostPipe *p = ctx->pipe;
    if (!p) return;
    for (hipStream_t s : {p->h2d, p->comp, p->d2h})
        if (s) hipStreamSynchronize(s);  // no chunk is in flight
    for (PipeSlot &sl : p->slots) {
        dfree_zeroed(ctx, sl.arena, p->chunk_bytes);
        dfree(ctx, sl.descs); dfree(ctx, sl.masks); dfree(ctx, sl.status);
        if (sl.h2d) hipEventDestroy(sl.h2d);
        if (sl.comp) hipEventDestroy(sl.comp);
        if (sl.d2h) hipEventDestroy(sl.d2h);
        sl = PipeSlot{};
    }
    p->slots.clear();
}

}  // namespace qpp

extern "C" {

// ---------------------------------------------------------------- batches

int qpp_seal_batch(qpp_ctx *ctx, const qpp_pkt *descs, size_t n, uint8_t *arena, uint8_t *masks, int8_t *status,
                   uint32_t flags, void *stream) {
    if (!ctx || (n && (!descs || !arena))) return QPP_INTERNAL_ERROR;
    if ((flags & QPP_HP_MASK_OUT) && !masks) return QPP_INTERNAL_ERROR;
    if (n > UINT32_MAX) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    // FIPS mode refuses out-of-order nonces per packet (the packet stays plaintext): without a status array the call
    // could not say which, so it is refused (the reference fails such an encrypt call: aead/fips.rs)
    if (ctx->fips_live && !status && !(flags & QPP_ONLY_CHACHA)) return QPP_INTERNAL_ERROR;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, stream, &st));
    RC_TRY(enqueue_batch(ctx, st, true, descs, (uint32_t)n, arena, masks, status, flags));
    return note_work(ctx, st);
}

int qpp_open_batch(qpp_ctx *ctx, const qpp_pkt *descs, size_t n, uint8_t *arena, int8_t *status, uint32_t flags,
                   void *stream) {
    if (!ctx || (n && (!descs || !arena || !status))) return QPP_INTERNAL_ERROR;
    if (n > UINT32_MAX) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, stream, &st));
    RC_TRY(enqueue_batch(ctx, st, false, descs, (uint32_t)n, arena, nullptr, status, flags));
    return note_work(ctx, st);
}

int qpp_unprotect_open_batch(qpp_ctx *ctx, const qpp_rx_pkt *rx, size_t n, uint8_t *arena, qpp_pkt *descs_out,
                             int8_t *status, uint32_t flags, void *stream) {
    if (!ctx || (n && (!rx || !arena || !descs_out || !status))) return QPP_INTERNAL_ERROR;
    if (n > UINT32_MAX) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, stream, &st));
    // Any live AES packet key (any number of them, both sizes, beside ChaCha20 keys, any header-key suite) and a batch
    // of the quad kernel's size: ONE fused cooperative launch -- unprotect, group by the chosen key, open the AES
    // packets (quad.hip) -- and, when ChaCha20 packet keys are live, the ChaCha20 packets it sorted out opened by one
    // more launch on the same stream (no host round trip).  The same outputs as the launches below.  QPP_RX_FUSED=0
    // forces the multi-launch path (A/B, tests).
    const char *fz = getenv("QPP_RX_FUSED");
    const uint32_t a128 = ctx->live_by_suite[QPP_SUITE_TLS_AES_128_GCM_SHA256],
                   a256 = ctx->live_by_suite[QPP_SUITE_TLS_AES_256_GCM_SHA384];
    const bool chacha = !(flags & QPP_ONLY_AES) && ctx->live_by_suite[QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256];
    if (!(flags & QPP_ONLY_CHACHA) && !(fz && fz[0] == '0') && a128 + a256 > 0 &&
        aes_path(ctx, (uint32_t)n) == AesPath::quad && ctx->key_cap <= quad_rx_max_keys()) {
        RC_TRY(ensure_plan(ctx, st, (uint32_t)n));  // perm
        const uint32_t kc = ctx->key_cap;
        if (st->rx_scratch_keys < kc)
            RC_TRY(regrow(ctx, st->stream, &st->rx_scratch, &st->rx_scratch_keys,
                          4 * (16 + 2 * (size_t)kc + 4 + 4 * ((size_t)kc + 1)), kc));
        HIP_TRY(ctx, hipMemsetAsync(st->rx_scratch, 0, 4 * (16 + 2 * (size_t)kc), st->stream));
        {
            // The grid barriers need every workgroup resident: the grid is the CUs every resident server of the
            // device leaves, the device's previous fused receive is waited for (two at once would split the CUs), and
            // a server launched later waits for this one (srv_start) -- all under the device registry's lock
            DevServers &r = dev_servers(ctx->device);
            std::lock_guard<std::mutex> lk(r.mu);
            if (!r.rx_tail) HIP_TRY(ctx, hipEventCreateWithFlags(&r.rx_tail, hipEventDisableTiming));
            else HIP_TRY(ctx, hipStreamWaitEvent(st->stream, r.rx_tail, 0));
            const uint32_t busy = resident_wgs_locked(r), free_cu = ctx->n_cu > busy ? ctx->n_cu - busy : 1u;
            const uint32_t grid = std::min<uint32_t>(free_cu, std::max<uint32_t>(1, (uint32_t)((n + 191) / 192)));
            HIP_TRY(ctx, launch_aes_gcm_quad_rx(a256 ? (a128 ? 0u : 14u) : 10u, grid, st->stream, ctx->d_keys, kc, rx,
                                                (uint32_t)n, arena, descs_out, status, st->rx_scratch, st->plan.perm,
                                                ctx->d_diag, chacha, ctx->pow));
            HIP_TRY(ctx, hipEventRecord(r.rx_tail, st->stream));
        }
        if (chacha)
            HIP_TRY(ctx, launch_chacha_sel(ctx->d_keys, kc, descs_out, (uint32_t)n, arena, status, st->plan.perm,
                                           st->rx_scratch + 2, st->stream));
        return note_work(ctx, st);
    }
    // No AES record live at all (packet or header keys): every header and packet key a packet can name is ChaCha20,
    // so the ChaCha lane kernel unprotects and opens in ONE launch, whatever the key mix (per-lane keys, no plan).
    const bool no_aes = !ctx->live_by_suite[QPP_SUITE_TLS_AES_128_GCM_SHA256] &&
                        !ctx->live_by_suite[QPP_SUITE_TLS_AES_256_GCM_SHA384] &&
                        !ctx->hdr_live_by_suite[QPP_SUITE_TLS_AES_128_GCM_SHA256] &&
                        !ctx->hdr_live_by_suite[QPP_SUITE_TLS_AES_256_GCM_SHA384];
    if (no_aes && !(flags & QPP_ONLY_AES) && !(fz && fz[0] == '0') && n > (ctx->burst_max >> kChachaBurstShift)) {
        HIP_TRY(ctx, launch_chacha_rx(ctx->d_keys, ctx->key_cap, rx, (uint32_t)n, arena, descs_out, status, st->stream));
        return note_work(ctx, st);
    }
    // 1. header unprotection + PN expansion + key-phase choice -> descs_out (device); 2. the open kernels on them,
    // grouped by the chosen key like any batch (skipped packets keep their DECODE_ERROR status)
    HIP_TRY(ctx, launch_unprotect(ctx->d_keys, ctx->key_cap, rx, (uint32_t)n, arena, descs_out, status, st->stream));
    RC_TRY(enqueue_batch(ctx, st, false, descs_out, (uint32_t)n, arena, nullptr, status, flags));
    return note_work(ctx, st);
}

int qpp_pn_truncate(uint64_t pn, uint64_t largest_acked, uint64_t *truncated, size_t *pn_len) {
    // derive_truncation_range: (pn - largest) * 2 must fit the 1..4-byte encoding (mod.rs:81-93, packet_number_len.rs:163-172)
    if (!truncated || !pn_len) return QPP_INTERNAL_ERROR;
    pn &= kPnMask;
    largest_acked &= kPnMask;
    if (pn < largest_acked) return QPP_DECODE_ERROR;
    const uint64_t range = (pn - largest_acked) * 2;
    size_t len = 0;
    for (size_t b = 1; b <= 4 && !len; b++)
        if (range <= (1ull << (8 * b)) - 1) len = b;
    if (!len) return QPP_DECODE_ERROR;
    *pn_len = len;
    *truncated = pn & ((1ull << (8 * len)) - 1);
    return QPP_OK;
}

uint64_t qpp_pn_expand(uint64_t largest_acked, uint64_t truncated, size_t pn_len) {
    if (pn_len < 1 || pn_len > 4) return UINT64_MAX;
    return decode_packet_number(largest_acked & kPnMask, truncated, (uint32_t)(8 * pn_len));
}

int qpp_hp_mask_batch(qpp_ctx *ctx, const qpp_pkt *descs, size_t n, const uint8_t *arena, uint8_t *masks,
                      void *stream) {
    if (!ctx || (n && (!descs || !arena || !masks))) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, stream, &st));
    HIP_TRY(ctx, launch_hp_mask(ctx->d_keys, ctx->key_cap, descs, (uint32_t)n, arena, masks, st->stream));
    return note_work(ctx, st);
}

// ---------------------------------------------------------------- host pipeline (packets start and end in host memory)

int qpp_ctx_set_host_pipe(qpp_ctx *ctx, size_t chunk_packets, size_t chunk_bytes, size_t slots) {
    if (!ctx || !chunk_packets || chunk_packets > UINT32_MAX || chunk_bytes < 4096 || slots < 2 || slots > 16)
        return QPP_INTERNAL_ERROR;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(servers_stop(ctx));
    RC_TRY(ctx_sync(ctx));
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    pipe_release(ctx);
    ctx->pipe->chunk_packets = chunk_packets;
    ctx->pipe->chunk_bytes = chunk_bytes;
    ctx->pipe->nslots = slots;
    ctx->pipe->auto_chunk = false;
    return QPP_OK;
}

int qpp_host_batch_submit(qpp_ctx *ctx, const qpp_pkt *descs, size_t n, uint8_t *arena, uint8_t *masks,
                          int8_t *status, uint32_t flags, uint32_t ops, uint64_t *ticket) {
    if (!ctx || !ticket || (n && (!descs || !arena))) return QPP_INTERNAL_ERROR;
    if (!(ops & (QPP_OP_SEAL | QPP_OP_OPEN)) || (ops & ~(QPP_OP_SEAL | QPP_OP_OPEN))) return QPP_INTERNAL_ERROR;
    if ((flags & QPP_HP_MASK_OUT) && !(masks && (ops & QPP_OP_SEAL))) return QPP_INTERNAL_ERROR;
    if ((ops & QPP_OP_OPEN) && n && !status) return QPP_INTERNAL_ERROR;
    if ((ops & QPP_OP_SEAL) && n && !status && ctx->fips_live && !(flags & QPP_ONLY_CHACHA))
        return QPP_INTERNAL_ERROR;  // FIPS refusals are reported per packet (qpp_seal_batch)
    if ((ops & QPP_OP_SEAL) && (ops & QPP_OP_OPEN) && (flags & QPP_HP_APPLY)) return QPP_INTERNAL_ERROR;
    const bool by_conn = (flags & QPP_KEY_BY_CONN) != 0;
    if (by_conn && !ctx->connmap_n) return QPP_INTERNAL_ERROR;  // no connection table
    flags &= ~QPP_KEY_BY_CONN;
    *ticket = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    HostPipe *p = ctx->pipe;
    RC_TRY(pipe_init(ctx));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, p->comp, &st));
    // chunks of consecutive packets: at most chunk_packets, span [lo, hi) of at most chunk_bytes; packets must be in
    // ascending, non-overlapping arena order so that spans of different chunks never overlap
    size_t cap = p->chunk_packets;
    if (p->auto_chunk) {
        const size_t keys = ctx->live_by_suite[QPP_SUITE_TLS_AES_128_GCM_SHA256] +
                            ctx->live_by_suite[QPP_SUITE_TLS_AES_256_GCM_SHA384];
        cap = std::min(p->chunk_packets, std::max<size_t>({(n + 15) / 16, 65536, 64 * keys}));
    }
    size_t i = 0;
    uint64_t prev_end = 0;
    while (i < n) {
        const size_t first = i;
        const uint64_t lo = descs[i].off;
        uint64_t hi = lo;
        while (i < n && i - first < cap) {
            const qpp_pkt &d = descs[i];
            const uint64_t end = (uint64_t)d.off + d.aad_len + d.pt_len + 16;
            if (d.off < prev_end) return QPP_INTERNAL_ERROR;  // out of order or overlapping
            if (end - lo > p->chunk_bytes) {
                if (i == first) return QPP_INTERNAL_ERROR;  // one packet larger than a chunk buffer
                break;
            }
            hi = std::max(hi, end);
            prev_end = end;
            i++;
        }
        const uint32_t cn = (uint32_t)(i - first);
        PipeSlot &sl = p->slots[p->next];
        p->next = (p->next + 1) % p->slots.size();
        // the slot's previous chunk must be back in host memory before its buffers are overwritten (device-side wait)
        if (sl.busy) HIP_TRY(ctx, hipStreamWaitEvent(p->h2d, sl.d2h, 0));
        HIP_TRY(ctx, hipMemcpyAsync(sl.arena, arena + lo, hi - lo, hipMemcpyHostToDevice, p->h2d));
        HIP_TRY(ctx, hipMemcpyAsync(sl.descs, descs + first, sizeof(qpp_pkt) * cn, hipMemcpyHostToDevice, p->h2d));
        HIP_TRY(ctx, hipEventRecord(sl.h2d, p->h2d));
        HIP_TRY(ctx, hipStreamWaitEvent(p->comp, sl.h2d, 0));
        if (by_conn)
            HIP_TRY(ctx, launch_conn_remap(sl.descs, cn, ctx->d_connmap, (uint32_t)ctx->connmap_n, p->comp));
        uint8_t *base = sl.arena - lo;  // descriptor offsets stay absolute: the kernels address base + off
        if (ops & QPP_OP_SEAL)
            RC_TRY(enqueue_batch(ctx, st, true, sl.descs, cn, base, sl.masks,
                                 (ops & QPP_OP_OPEN) ? nullptr : sl.status, flags));
        if (ops & QPP_OP_OPEN)
            RC_TRY(enqueue_batch(ctx, st, false, sl.descs, cn, base, nullptr, sl.status,
                                 flags & ~(QPP_HP_MASK_OUT | QPP_HP_APPLY)));
        HIP_TRY(ctx, hipEventRecord(sl.comp, p->comp));
        HIP_TRY(ctx, hipStreamWaitEvent(p->d2h, sl.comp, 0));
        HIP_TRY(ctx, hipMemcpyAsync(arena + lo, sl.arena, hi - lo, hipMemcpyDeviceToHost, p->d2h));
        if ((flags & QPP_HP_MASK_OUT) && masks)
            HIP_TRY(ctx, hipMemcpyAsync(masks + 5 * first, sl.masks, 5 * (size_t)cn, hipMemcpyDeviceToHost, p->d2h));
        if (status) HIP_TRY(ctx, hipMemcpyAsync(status + first, sl.status, cn, hipMemcpyDeviceToHost, p->d2h));
        HIP_TRY(ctx, hipEventRecord(sl.d2h, p->d2h));
        sl.busy = true;
    }
    RC_TRY(note_work(ctx, st));
    hipEvent_t done = get_event(ctx);
    if (!done) return QPP_DEVICE_ERROR;
    HIP_TRY(ctx, hipEventRecord(done, p->d2h));
    *ticket = p->next_ticket++;
    p->tickets[*ticket] = done;
    return QPP_OK;
}

int qpp_ctx_set_conn_keys(qpp_ctx *ctx, const uint32_t *slots, size_t n) {
    if (!ctx || !n || !slots || n > UINT32_MAX) return QPP_INTERNAL_ERROR;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    RC_TRY(pipe_init(ctx));
    hipStream_t s = ctx->pipe->comp;  // the remap launches' stream: earlier batches read the old table first
    if (n > ctx->connmap_cap) {
        const size_t cap = std::max<size_t>(n, 1024);
        ctx->connmap_n = 0;  // (no table until the copy below)
        // freed behind every stream (dfree): conn-keyed batches of any stream read it
        RC_TRY(regrow(ctx, s, &ctx->d_connmap, &ctx->connmap_cap, 4 * cap, cap));
    }
    // through the pinned stage: the caller may reuse `slots` on return (the previous copy from the stage is waited
    // for first -- a host wait only when two tables are swapped back to back)
    if (!ctx->connstage_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->connstage_ev, hipEventDisableTiming));
    if (ctx->connstage_used) HIP_TRY(ctx, hipEventSynchronize(ctx->connstage_ev));
    ctx->connstage_used = false;
    if (n > ctx->connstage_cap) {
        hfree(ctx, ctx->h_connstage);
        ctx->h_connstage = nullptr;
        ctx->connstage_cap = 0;
        const size_t cap = std::max<size_t>(n, 1024);
        HIP_TRY(ctx, hmalloc(&ctx->h_connstage, 4 * cap, hipHostMallocDefault));
        ctx->connstage_cap = cap;
    }
    memcpy(ctx->h_connstage, slots, 4 * n);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_connmap, ctx->h_connstage, 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ctx->connstage_ev, s));
    ctx->connstage_used = true;
    ctx->connmap_n = n;
    return QPP_OK;
}

int qpp_host_batch_query(qpp_ctx *ctx, uint64_t ticket, int *done) {
    if (!ctx || !done || !ctx->pipe) return QPP_INTERNAL_ERROR;
    auto it = ctx->pipe->tickets.find(ticket);
    if (it == ctx->pipe->tickets.end()) return QPP_INTERNAL_ERROR;
    const hipError_t q = hipEventQuery(it->second);
    if (q == hipErrorNotReady) { *done = 0; return QPP_OK; }
    HIP_TRY(ctx, q);
    *done = 1;
    return QPP_OK;
}

int qpp_host_batch_wait(qpp_ctx *ctx, uint64_t ticket) {
    if (!ctx || !ctx->pipe) return QPP_INTERNAL_ERROR;
    auto it = ctx->pipe->tickets.find(ticket);
    if (it == ctx->pipe->tickets.end()) return QPP_INTERNAL_ERROR;
    hipEvent_t e = it->second;
    ctx->pipe->tickets.erase(it);
    const hipError_t r = hipEventSynchronize(e);
    put_event(ctx, e);
    HIP_TRY(ctx, r);
    return QPP_OK;
}

}  // extern "C"
