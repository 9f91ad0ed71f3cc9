// packet.cpp -- the per-packet calls (Key::encrypt / Key::decrypt / header-protection mask of one packet): through the
// context's packet server without a launch, else a batch of one on the pinned stage.
#include "host.h"

namespace qpp {

// per-packet staging: the pinned stage the launched path runs on in place, and its device twin
static int ensure_stage(qpp_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->stage_cap) return QPP_OK;
    size_t cap = std::max<size_t>(4096, ctx->stage_cap);
    while (cap < bytes) cap *= 2;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    dfree(ctx, ctx->d_stage);
    hfree(ctx, ctx->h_stage);
    ctx->d_stage = ctx->h_stage = ctx->v_stage = nullptr;
    ctx->stage_cap = 0;
    HIP_TRY(ctx, dmalloc(ctx, &ctx->d_stage, cap));
    HIP_TRY(ctx, hmalloc_mapped(&ctx->h_stage, &ctx->v_stage, cap, hipHostMallocDefault));
    ctx->stage_cap = cap;
    return QPP_OK;
}

// Key::encrypt / Key::decrypt (crypto/src/packet_protection.rs; cipher_suite.rs:86-160) of one packet through the
// context's packet server: the header and payload (and the tag, to open) are copied into its pinned ring, posted as
// one work item to workgroup slot % kPktWgs (so a connection's sealer and opener keep their GHASH tables in different
// workgroups' LDS), sealed without header protection or opened in place there, and copied back.  No launch, no
// runtime call: the cost is the post's PCIe round trip, the packet's own read / AES / GHASH / write chain and the copies.
constexpr size_t kPktRing = 16384;  // header + payload + tag; longer packets take the launched path
// zeroes the packet server's ring bytes of a call on every exit path (an early return left plaintext there)
struct RingWipe {
    uint8_t *p;
    size_t n;
    ~RingWipe() { secure_zero(p, n); }
};
constexpr uint32_t kPktWgs = 4;

// Posts one work item (rounds nr) of one packet d (ring offset 0) to workgroup wg of the packet server -- every other
// workgroup an empty item -- and waits for it.  The slot's status byte is preset to INTERNAL_ERROR (left so if the
// record is not what the item names).
static int srv_post_one(qpp_txq *q, std::chrono::steady_clock::time_point now, uint32_t wg, uint32_t nr,
                        const qpp_pkt &d) {
    RC_TRY(srv_start(q, true));  // (the caller found it a server slot)
    q->srv_seq = srv_next(q->srv_seq);
    const uint32_t seq = q->srv_seq;
    const uint32_t word = (q->srv_epoch << 24) | q->srv_wgs;  // item b for workgroup b; all but one empty
    q->h_slots[wg].status[0] = (int8_t)QPP_INTERNAL_ERROR;
    for (uint32_t b = 0; b < q->srv_wgs; b++)
        srv_write_slot(q->h_slots[b], seq, word, b == wg ? WorkItem{d.key_idx, 0, 1, nr} : WorkItem{0, 0, 0, 0}, &d);
    q->srv_last_post = now;
    q->srv_posted = seq;
    q->srv_first = q->srv_last = 0;  // (no ticket: nothing of the transmit-queue API refers to this post)
    q->n_server++;
    q->ctx->pkt_calls++;
    return srv_wait(q, seq);
}

// The context's packet server (created on the first call) ready for a post at *now: pending key records installed, the
// previous post done, the server running.  kNoServerSlot: every server slot of the device is taken
static int packet_server_ready(qpp_ctx *ctx, qpp_txq **q, std::chrono::steady_clock::time_point *now) {
    if (!ctx->pkt_q) RC_TRY(txq_create_server(ctx, kPktRing, 1, kPktWgs, &ctx->pkt_q));
    *q = ctx->pkt_q;
    RC_TRY(flush_keys(ctx));
    *now = std::chrono::steady_clock::now();
    RC_TRY(srv_prepare(*q, *now));
    return srv_start(*q);
}

// *handled = false: the call is not one the server takes (FIPS seal, packet over kPktRing, server off, no server slot)
// -- the caller launches it
static int packet_server_run(const qpp_key *k, bool seal, uint64_t pn, const uint8_t *header, size_t header_len,
                             const uint8_t *payload, size_t payload_len, uint8_t *out, uint8_t *tag_out,
                             int8_t *status_out, bool *handled) {
    qpp_ctx *ctx = k->ctx;
    *handled = false;
    const DevKey &rec = ctx->h_keys[k->slot];
    const size_t total = header_len + payload_len + 16;
    // FIPS seals keep the launched path (its nonce-order gate)
    if (!ctx->pkt_server || (seal && rec.fips) || total > kPktRing) return QPP_OK;
    qpp_txq *q = nullptr;
    std::chrono::steady_clock::time_point now;
    if (const int rc = packet_server_ready(ctx, &q, &now)) return rc == kNoServerSlot ? QPP_OK : rc;
    uint8_t *r = q->h_ring;
    RingWipe wipe{r, total};  // the plaintext never stays in the host-visible ring, whatever the exit path
    if (header_len) memcpy(r, header, header_len);
    if (payload_len) memcpy(r + header_len, payload, payload_len);
    if (!seal) memcpy(r + header_len + payload_len, tag_out, 16);
    const uint32_t wg = k->slot % q->srv_wgs;
    RC_TRY(srv_post_one(q, now, wg, rec.nr, qpp_pkt{pn, k->slot, 0, (uint16_t)header_len, (uint16_t)payload_len, 0,
                                                    uint8_t(seal ? kTxsPktNoHp : kTxsPktOpen), 0}));
    *status_out = __atomic_load_n(&q->h_slots[wg].status[0], __ATOMIC_ACQUIRE);
    *handled = true;
    if (!(seal && *status_out != QPP_OK)) {  // (a refused seal leaves the caller's buffer untouched)
        memcpy(out, r + header_len, payload_len);
        if (seal) memcpy(tag_out, r + header_len + payload_len, 16);
    }
    return QPP_OK;
}

// HeaderKey::*_header_protection_mask of one sample (header_key.rs:52-56) through the packet server: the sample at
// ring offset 0, the mask written at 16 by a mask item (kTxsMaskNr) on workgroup slot % kPktWgs
// (*handled = false: server off, or no server slot)
static int packet_server_mask(qpp_ctx *ctx, uint32_t slot, const uint8_t *sample, uint8_t mask[5], bool *handled) {
    *handled = false;
    if (!ctx->pkt_server || slot >= ctx->key_cap || !ctx->h_keys[slot].live) return QPP_OK;
    qpp_txq *q = nullptr;
    std::chrono::steady_clock::time_point now;
    if (const int rc = packet_server_ready(ctx, &q, &now)) return rc == kNoServerSlot ? QPP_OK : rc;
    uint8_t *r = q->h_ring;
    RingWipe wipe{r, 32};
    memcpy(r, sample, 16);
    memset(r + 16, 0, 16);
    RC_TRY(srv_post_one(q, now, slot % q->srv_wgs, kTxsMaskNr, qpp_pkt{0, slot, 0, 16, 0, 0, 0, 0}));
    memcpy(mask, r + 16, 5);
    *handled = true;
    return QPP_OK;
}

// One packet through the batch kernels, zero-copy: the kernel reads and writes the pinned stage directly (no DMA
// copies; one launch, one wait).  Stage layout: descriptor @0 | perm @32 | plan meta @36 (4 words) | work item @52
// | status @72 | mask @80 | packet @kOnePkt = [pad 16 | header | payload | tag].
constexpr size_t kOnePkt = 128;
static int run_one(const qpp_key *k, bool seal, uint64_t pn, const uint8_t *header, size_t header_len,
                   const uint8_t *payload, size_t payload_len, uint8_t *out, uint8_t *tag_out, int8_t *status_out) {
    qpp_ctx *ctx = k->ctx;
    if (header_len > 0xffff || payload_len > 0xffff) return QPP_INTERNAL_ERROR;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool handled = false;
    RC_TRY(packet_server_run(k, seal, pn, header, header_len, payload, payload_len, out, tag_out, status_out, &handled));
    if (handled) return QPP_OK;
    const size_t total = kOnePkt + 16 + header_len + payload_len + 16;
    RC_TRY(ensure_stage(ctx, total));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, nullptr, &st));
    uint8_t *h = ctx->h_stage, *v = ctx->v_stage;
    memset(h, 0, total);
    uint8_t *pkt = h + kOnePkt;
    memcpy(pkt + 16, header, header_len);
    memcpy(pkt + 16 + header_len, payload, payload_len);
    if (!seal) memcpy(pkt + 16 + header_len + payload_len, tag_out, 16);
    qpp_pkt &d = *(qpp_pkt *)h;
    d.pn = pn;
    d.key_idx = k->slot;
    d.off = 16;
    d.aad_len = (uint16_t)header_len;
    d.pt_len = (uint16_t)payload_len;
    const uint32_t nr = ctx->h_keys[k->slot].nr;
    *(uint32_t *)(h + 32) = 0;  // perm = {0}
    uint32_t *meta = (uint32_t *)(h + 36);  // one work item, on this key, in its AES size's class
    meta[0] = 1;
    meta[1] = nr == 10 ? 1 : 0;
    meta[2] = nr == 10 ? 1 : 0;
    meta[3] = nr == 10 ? 0 : 1;
    *(WorkItem *)(h + 52) = WorkItem{k->slot, 0, 1, nr};
    h[72] = (uint8_t)QPP_INTERNAL_ERROR;  // overwritten by the kernel
    PlanBuffers pb{};
    pb.perm = (uint32_t *)(v + 32);
    pb.work = (WorkItem *)(v + 52);
    pb.n_work = (uint32_t *)(v + 36);
    hipStream_t s = ctx->stream;
    const qpp_pkt *vd = (const qpp_pkt *)v;
    int8_t *vst = (int8_t *)(v + 72);
    if (seal && ctx->h_keys[k->slot].fips) {  // FIPS mode: the nonce-order gate (refused: status INTERNAL_ERROR)
        RC_TRY(fips_gate(ctx, st, vd, 1, vst, nullptr));
    }
    if (is_aes(k->suite)) {
        // key_cap = 0: grid = plan_max_work(1, 0, per) = 1; only work item 0 exists
        if (ctx->burst_max)
            HIP_TRY(ctx, launch_aes_gcm_burst(seal, ctx->d_keys, vd, pb, 1, 0, 1, v + kOnePkt, v + 80, vst, 0,
                                              1u << k->suite, ctx->pow, s));
        else
            HIP_TRY(ctx, launch_aes_gcm(seal, ctx->d_keys, vd, pb, 1, 1, v + kOnePkt, v + 80, vst, 0, 1u << k->suite,
                                        ctx->pow, s));
    } else {
        HIP_TRY(ctx, launch_chacha(seal, ctx->d_keys, ctx->key_cap, vd, 1, v + kOnePkt, v + 80, vst, 0,
                                   ctx->burst_max > 0, s));
    }
    RC_TRY(note_work(ctx, st));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    *status_out = (int8_t)h[72];
    if (seal && *status_out != QPP_OK) {  // refused (FIPS nonce order): the caller's buffer stays untouched
        secure_zero(h, total);
        return QPP_OK;
    }
    memcpy(out, pkt + 16 + header_len, payload_len);
    if (seal) memcpy(tag_out, pkt + 16 + header_len + payload_len, 16);
    secure_zero(h, total);
    return QPP_OK;
}

// HeaderKey::*_header_protection_mask for one sample through the hp_mask kernel, zero-copy on the pinned stage:
// descriptor @0, sample @64 (+4), mask @96.
static int mask_one(qpp_ctx *ctx, uint32_t slot, const uint8_t *sample, uint8_t mask[5]) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool handled = false;
    RC_TRY(packet_server_mask(ctx, slot, sample, mask, &handled));
    if (handled) return QPP_OK;
    RC_TRY(ensure_stage(ctx, 128));
    RC_TRY(flush_keys(ctx));
    StreamState *st = nullptr;
    RC_TRY(batch_stream(ctx, nullptr, &st));
    uint8_t *h = ctx->h_stage;
    memset(h, 0, 128);
    memcpy(h + 64 + 4, sample, 16);
    qpp_pkt &d = *(qpp_pkt *)h;
    d.key_idx = slot;  // off = aad_len = pn_len = 0: sample at offset 4
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, launch_hp_mask(ctx->d_keys, ctx->key_cap, (const qpp_pkt *)ctx->v_stage, 1, ctx->v_stage + 64,
                                ctx->v_stage + 96, s));
    RC_TRY(note_work(ctx, st));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(mask, h + 96, 5);
    return QPP_OK;
}

}  // namespace qpp

extern "C" {

// ---------------------------------------------------------------- per packet

int qpp_seal(qpp_key *key, uint64_t pn, const uint8_t *header, size_t header_len, uint8_t *payload, size_t payload_len,
             size_t payload_cap) {
    if (!key || (!header && header_len) || (!payload && payload_len)) return QPP_INTERNAL_ERROR;
    if (payload_cap < payload_len + 16) return QPP_INTERNAL_ERROR;
    int8_t st;
    int rc = run_one(key, true, pn, header, header_len, payload, payload_len, payload, payload + payload_len, &st);
    return rc ? rc : st;
}

int qpp_seal_scatter(qpp_key *key, uint64_t pn, const uint8_t *header, size_t header_len, uint8_t *in_out,
                     size_t in_len, const uint8_t *extra_in, size_t extra_len, uint8_t *extra_out_and_tag) {
    if (!key || (!in_out && in_len) || (!extra_in && extra_len) || !extra_out_and_tag) return QPP_INTERNAL_ERROR;
    std::vector<uint8_t> flat(in_len + extra_len);
    if (in_len) memcpy(flat.data(), in_out, in_len);
    if (extra_len) memcpy(flat.data() + in_len, extra_in, extra_len);
    int8_t st;
    int rc = run_one(key, true, pn, header, header_len, flat.data(), flat.size(), flat.data(), extra_out_and_tag + extra_len, &st);
    if (!rc) {
        if (in_len) memcpy(in_out, flat.data(), in_len);
        if (extra_len) memcpy(extra_out_and_tag, flat.data() + in_len, extra_len);
    }
    secure_zero(flat.data(), flat.size());
    return rc ? rc : st;
}

int qpp_open(const qpp_key *key, uint64_t pn, const uint8_t *header, size_t header_len, uint8_t *payload,
             size_t payload_len) {
    if (!key || (!header && header_len) || (!payload && payload_len)) return QPP_INTERNAL_ERROR;
    if (payload_len < 16) return QPP_DECRYPT_ERROR;  // cipher_suite.rs:126-129
    uint8_t tag[16];
    memcpy(tag, payload + payload_len - 16, 16);
    int8_t st;
    int rc = run_one(key, false, pn, header, header_len, payload, payload_len - 16, payload, tag, &st);
    return rc ? rc : st;
}

int qpp_hp_mask(const qpp_key *key, const uint8_t *sample, size_t sample_len, uint8_t mask[5]) {
    if (!key || !sample || !mask || sample_len < 16) return QPP_INTERNAL_ERROR;
    return mask_one(key->ctx, key->slot, sample, mask);
}

int qpp_header_key_mask(const qpp_header_key *hk, const uint8_t *sample, size_t sample_len, uint8_t mask[5]) {
    if (!hk || !sample || !mask || sample_len < 16) return QPP_INTERNAL_ERROR;
    return mask_one(hk->ctx, hk->slot, sample, mask);
}

// ---------------------------------------------------------------- dc consumers (dc/s2n-quic-dc/src/crypto/awslc.rs)

int qpp_dc_seal(const qpp_key *key, uint64_t pn, const uint8_t *header, size_t header_len, const uint8_t *extra_payload,
                size_t extra_len, uint8_t *payload_and_tag, size_t len) {
    // awslc.rs:53-83: inline_len = len - tag - extra; seal_in_place_scatter(in_out = [0, inline), extra_out_and_tag)
    if (!key || (!header && header_len) || (!extra_payload && extra_len) || !payload_and_tag) return QPP_INTERNAL_ERROR;
    if (len < 16 || len - 16 < extra_len) return QPP_INTERNAL_ERROR;
    const size_t msg = len - 16, inline_len = msg - extra_len;
    int8_t st;
    int rc;
    if (!extra_len) {
        rc = run_one(key, true, pn, header, header_len, payload_and_tag, msg, payload_and_tag, payload_and_tag + msg, &st);
    } else {
        std::vector<uint8_t> flat(msg);  // inline || extra as one message; the sealed bytes land in payload_and_tag
        if (inline_len) memcpy(flat.data(), payload_and_tag, inline_len);
        memcpy(flat.data() + inline_len, extra_payload, extra_len);
        rc = run_one(key, true, pn, header, header_len, flat.data(), msg, payload_and_tag, payload_and_tag + msg, &st);
        secure_zero(flat.data(), flat.size());
    }
    return rc ? rc : st;
}

int qpp_dc_open(const qpp_key *key, int key_phase, uint64_t pn, const uint8_t *header, size_t header_len,
                const uint8_t *payload_in, const uint8_t *tag, size_t tag_len, uint8_t *payload_out, size_t payload_len) {
    // awslc.rs:176-204: ensure!(key_phase == Zero, RotationNotSupported); open_separate_gather -> InvalidTag
    if (!key || (!header && header_len) || ((!payload_in || !payload_out) && payload_len) || (!tag && tag_len))
        return QPP_INTERNAL_ERROR;
    if (key_phase != 0) return QPP_ROTATION_NOT_SUPPORTED;
    if (tag_len != 16) {
        if (payload_len) memset(payload_out, 0, payload_len);
        return QPP_DECRYPT_ERROR;
    }
    uint8_t t[16];
    memcpy(t, tag, 16);
    int8_t st;
    int rc = run_one(key, false, pn, header, header_len, payload_in, payload_len, payload_out, t, &st);
    return rc ? rc : st;
}

int qpp_dc_open_in_place(const qpp_key *key, int key_phase, uint64_t pn, const uint8_t *header, size_t header_len,
                         uint8_t *payload, size_t payload_len, const uint8_t *tag, size_t tag_len) {
    // awslc.rs:207-227: open_in_place_separate_tag
    if (!key || (!header && header_len) || (!payload && payload_len) || (!tag && tag_len)) return QPP_INTERNAL_ERROR;
    if (key_phase != 0) return QPP_ROTATION_NOT_SUPPORTED;
    if (tag_len != 16) return QPP_DECRYPT_ERROR;
    uint8_t t[16];
    memcpy(t, tag, 16);
    int8_t st;
    int rc = run_one(key, false, pn, header, header_len, payload, payload_len, payload, t, &st);
    return rc ? rc : st;
}

int qpp_ctx_set_packet_server(qpp_ctx *ctx, int on) {
    if (!ctx) return QPP_INTERNAL_ERROR;
    ctx->pkt_server = on != 0;
    if (!on && ctx->pkt_q) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        ctx->pkt_starts += ctx->pkt_q->n_starts;
        qpp_txq_destroy(ctx->pkt_q);
        ctx->pkt_q = nullptr;
    }
    return QPP_OK;
}

int qpp_ctx_packet_server_info(const qpp_ctx *ctx, uint64_t *calls, uint64_t *starts) {
    if (!ctx) return QPP_INTERNAL_ERROR;
    if (calls) *calls = ctx->pkt_calls;
    if (starts) *starts = ctx->pkt_starts + (ctx->pkt_q ? ctx->pkt_q->n_starts : 0);
    return QPP_OK;
}

}  // extern "C"
