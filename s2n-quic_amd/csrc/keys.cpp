// keys.cpp -- the device key table: slots, installs on the key stream, stream-ordered retirement, device-side
// derivation, and the key / header-key handles of the C ABI.
//
// Asynchrony rules (DESIGN.md §2 "Key lifetime"):
//   * every stream a batch is enqueued on gets a StreamState: its own plan scratch (two streams of one context never
//     share counts/perm/work) and an event recorded after its latest batch;
//   * key records reach HBM on the context's key stream (one install launch per flush, over a slot list, never a range
//     that could rewrite a live neighbour) and a `keys_ready` event; a batch on any stream first waits (device side)
//     for the latest install it has not yet waited for.  The host never blocks on data batches to install a key;
//   * a freed key's slot is retired in stream order on the retire stream: freed slots collect in a pending list that
//     is flushed before the next batch, key install or synchronisation (or once it holds kRetireFlush slots): the
//     retire stream waits for every StreamState's last event, one memset per run of consecutive slots zeroes their
//     device records, and one
//     "retired" event marks them; the slots are reused only once that completed.  (A rotation of 4096 keys used to
//     cost 4096 memset launches.)
#include "host.h"

namespace qpp {

int grow_keys(qpp_ctx *ctx, uint32_t need) {
    if (need <= ctx->key_cap) return QPP_OK;
    uint32_t cap = std::max<uint32_t>(64, ctx->key_cap);
    while (cap < need) cap *= 2;
    DevKey *nk = nullptr;
    RC_TRY(servers_stop(ctx));  // they hold the old table's address
    RC_TRY(ctx_sync(ctx));      // no batch may still read the old table
    HIP_TRY(ctx, dmalloc(ctx, &nk, sizeof(DevKey) * cap));
    // Stream-ordered and waited for: a plain hipMemset runs on the null stream, which does not order against the
    // context's non-blocking streams (a batch could read the table before it is zeroed).
    HIP_TRY(ctx, hipMemsetAsync(nk, 0, sizeof(DevKey) * cap, ctx->kstream));
    if (ctx->d_keys)
        HIP_TRY(ctx, hipMemcpyAsync(nk, ctx->d_keys, sizeof(DevKey) * ctx->key_cap, hipMemcpyDeviceToDevice,
                                    ctx->kstream));
    const uint32_t pcap = std::min<uint32_t>(cap, kPowSlots);
    uint8_t *np = ctx->pow.base;
    if (pcap > ctx->pow.cap) {  // the precomputed tables of the slots so far move along
        HIP_TRY(ctx, dmalloc(ctx, &np, (size_t)pcap * kPowBytes));
        if (ctx->pow.cap)
            HIP_TRY(ctx, hipMemcpyAsync(np, ctx->pow.base, (size_t)ctx->pow.cap * kPowBytes, hipMemcpyDeviceToDevice,
                                        ctx->kstream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->kstream));
    dfree_zeroed(ctx, ctx->d_keys, sizeof(DevKey) * ctx->key_cap);
    if (np != ctx->pow.base) {
        // powers of each key's H: zeroized before the old buffer goes back to the allocator, like the records
        dfree_zeroed(ctx, ctx->pow.base, (size_t)ctx->pow.cap * kPowBytes);
        ctx->pow = PowTables{np, pcap};
    }
    ctx->d_keys = nk;
    ctx->h_keys.resize(cap);
    ctx->dirty_flag.resize(cap, 0);
    ctx->key_cap = cap;
    return QPP_OK;
}

// The key stage for the next key-stream job, with room for `bytes`: the stage the previous job did not use, once
// ITS previous job has read it (host wait on that job's event only -- the other stage's job, e.g. the install that
// flush_keys just queued, keeps running).  The caller records release_kstage after enqueueing its copies.
static int take_kstage(qpp_ctx *ctx, size_t bytes, KStage **out) {
    KStage &k = ctx->kstage[ctx->kstage_next];
    ctx->kstage_next ^= 1;
    if (k.used) HIP_TRY(ctx, hipEventSynchronize(k.free_ev));
    k.used = false;
    if (k.pending) secure_zero(k.h, k.pending);
    k.pending = 0;
    if (!k.free_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&k.free_ev, hipEventDisableTiming));
    if (bytes > k.cap) {
        size_t cap = std::max<size_t>(1 << 16, k.cap);
        while (cap < bytes) cap *= 2;
        dfree(ctx, k.d);  // (its last job, the previous user of this stage, is done)
        if (k.h) { secure_zero(k.h, k.cap); hfree(ctx, k.h); }
        k.d = nullptr;
        k.h = nullptr;
        k.cap = 0;
        HIP_TRY(ctx, dmalloc(ctx, &k.d, cap));
        HIP_TRY(ctx, hmalloc(&k.h, cap, hipHostMallocDefault));
        k.cap = cap;
    }
    *out = &k;
    return QPP_OK;
}
// after the job's last read of the stage was enqueued on the key stream; `pending` bytes of h are zeroized later
static int release_kstage(qpp_ctx *ctx, KStage *k, size_t pending) {
    HIP_TRY(ctx, hipEventRecord(k->free_ev, ctx->kstream));
    k->used = true;
    k->pending = pending;
    return QPP_OK;
}

// Zeroizes the slots' device records behind every batch already enqueued on any stream of this context (one launch
// for all pending slots), then queues the slots for reuse (cipher_suite.rs:106-114,189-193 zeroize on drop; here
// "drop" is stream-ordered).  Called before anything new is enqueued, so the retire stream waits only for batches
// enqueued before the keys were freed (and possibly a few after: never too early).
int flush_retire(qpp_ctx *ctx) {
    if (ctx->retire_pending.empty()) return QPP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(servers_quiesce(ctx));  // a server flush in flight may still read the freed records
    for (StreamState *st : ctx->streams)
        if (st->used) HIP_TRY(ctx, hipStreamWaitEvent(ctx->rstream, st->last, 0));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->rstream, ctx->keys_ready, 0));  // behind the slots' own installs
    // one memset per run of consecutive slots (a rotation frees whole batches of keys that were allocated together)
    std::vector<uint32_t> sorted(ctx->retire_pending);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size();) {
        size_t j = i + 1;
        while (j < sorted.size() && sorted[j] == sorted[j - 1] + 1) j++;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_keys + sorted[i], 0, sizeof(DevKey) * (j - i), ctx->rstream));
        if (sorted[i] < ctx->pow.cap) {  // the burst power tables are derived from H: zeroized with the record
            const size_t k = std::min<size_t>(j - i, ctx->pow.cap - sorted[i]);
            HIP_TRY(ctx, hipMemsetAsync(ctx->pow.base + (size_t)sorted[i] * kPowBytes, 0, kPowBytes * k, ctx->rstream));
        }
        i = j;
    }
    hipEvent_t e = get_event(ctx);
    if (!e || hipEventRecord(e, ctx->rstream) != hipSuccess) {
        // no event: wait here instead (a slot must never be reused while a batch may read it)
        put_event(ctx, e);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->rstream));
        ctx->free_slots.insert(ctx->free_slots.end(), ctx->retire_pending.begin(), ctx->retire_pending.end());
        ctx->retire_pending.clear();
        return QPP_OK;
    }
    ctx->retired_slots += (uint32_t)ctx->retire_pending.size();
    ctx->retired.push_back(Retired{std::move(ctx->retire_pending), e});
    ctx->retire_pending.clear();
    return QPP_OK;
}

int flush_keys(qpp_ctx *ctx) {
    RC_TRY(flush_retire(ctx));
    if (ctx->dirty.empty()) return QPP_OK;
    const uint32_t n = (uint32_t)ctx->dirty.size();
    const size_t rec = sizeof(DevKey) * n, slots = 4 * (size_t)n;
    KStage *k = nullptr;
    RC_TRY(take_kstage(ctx, rec + slots, &k));
    for (uint32_t i = 0; i < n; i++) {
        memcpy(k->h + sizeof(DevKey) * i, &ctx->h_keys[ctx->dirty[i]], sizeof(DevKey));
        ctx->dirty_flag[ctx->dirty[i]] = 0;
    }
    memcpy(k->h + rec, ctx->dirty.data(), slots);
    hipStream_t s = ctx->kstream;
    HIP_TRY(ctx, hipMemcpyAsync(k->d, k->h, rec + slots, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_key_install(ctx->d_keys, (const uint32_t *)(k->d + rec), (const DevKey *)k->d, n, ctx->pow, s));
    HIP_TRY(ctx, hipMemsetAsync(k->d, 0, rec, s));
    HIP_TRY(ctx, hipEventRecord(ctx->keys_ready, s));
    ctx->key_gen++;
    ctx->dirty.clear();
    // the pinned copy of the records is zeroized when the stage is next taken (its copy is done by then)
    return release_kstage(ctx, k, rec);
}

static void mark_dirty(qpp_ctx *ctx, uint32_t slot) {
    if (!ctx->dirty_flag[slot]) {
        ctx->dirty_flag[slot] = 1;
        ctx->dirty.push_back(slot);
    }
}

// A slot for a new key: a retired slot whose zeroing has completed, else a fresh one.
static int alloc_slot(qpp_ctx *ctx, uint32_t *out) {
    RC_TRY(flush_retire(ctx));
    while (!ctx->retired.empty()) {
        const hipError_t q = hipEventQuery(ctx->retired.front().done);
        if (q == hipErrorNotReady) break;
        if (fail(ctx, q, "retired slot event")) return QPP_DEVICE_ERROR;
        Retired &r = ctx->retired.front();
        ctx->free_slots.insert(ctx->free_slots.end(), r.slots.rbegin(), r.slots.rend());
        ctx->retired_slots -= (uint32_t)r.slots.size();
        put_event(ctx, r.done);
        ctx->retired.pop_front();
    }
    if (!ctx->free_slots.empty()) {
        *out = ctx->free_slots.back();
        ctx->free_slots.pop_back();
        return QPP_OK;
    }
    RC_TRY(grow_keys(ctx, ctx->next_slot + 1));
    *out = ctx->next_slot++;
    return QPP_OK;
}

// Frees a slot: the host copy is zeroized now, the device record behind in-flight work (flush_retire).
static void retire_slot(qpp_ctx *ctx, uint32_t slot) {
    secure_zero(&ctx->h_keys[slot], sizeof(DevKey));
    ctx->retire_pending.push_back(slot);
    if (ctx->retire_pending.size() >= kRetireFlush) flush_retire(ctx);
}

// Fills the slot's host record from the key's material and marks it for installation.
static int install(qpp_key *k) {
    qpp_ctx *ctx = k->ctx;
    RC_TRY(alloc_slot(ctx, &k->slot));
    DevKey &d = ctx->h_keys[k->slot];
    memset(&d, 0, sizeof d);
    d.suite = (uint32_t)k->suite;
    d.live = 1;
    memcpy(d.iv, k->iv, 12);
    if (k->suite == QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256) {
        memcpy(d.rk, k->key, 32);
        memcpy(d.hp_rk, k->hp, 32);
    } else {
        const size_t kl = suite_key_len(k->suite);
        d.nr = (uint32_t)aes_expand_key(k->key, kl, d.rk);
        d.hp_nr = (uint32_t)aes_expand_key(k->hp, kl, d.hp_rk);
    }
    d.fips = ctx->fips && is_aes(k->suite) ? 1u : 0u;  // no FIPS ChaCha20-Poly1305 (cipher_suite/ring.rs:116-121)
    ctx->fips_live += d.fips;
    mark_dirty(ctx, k->slot);
    ctx->live_by_suite[k->suite]++;
    ctx->live_slot_xor ^= k->slot;
    return QPP_OK;
}

static int install_header(qpp_header_key *h) {
    qpp_ctx *ctx = h->ctx;
    RC_TRY(alloc_slot(ctx, &h->slot));
    DevKey &d = ctx->h_keys[h->slot];
    memset(&d, 0, sizeof d);
    d.suite = (uint32_t)h->suite;
    d.live = 2;  // header key only: no packet key, never planned or sealed with
    if (h->suite == QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256) memcpy(d.hp_rk, h->hp, 32);
    else d.hp_nr = (uint32_t)aes_expand_key(h->hp, suite_key_len(h->suite), d.hp_rk);
    ctx->hdr_live_by_suite[h->suite & 3]++;
    mark_dirty(ctx, h->slot);
    return QPP_OK;
}

static void derive(qpp_key *k) {
    const size_t hl = suite_hash_len(k->suite), kl = suite_key_len(k->suite);
    hkdf_expand_label(hl, k->secret, "quic key", k->key, kl);
    hkdf_expand_label(hl, k->secret, "quic iv", k->iv, 12);
    hkdf_expand_label(hl, k->secret, "quic hp", k->hp, kl);
}

// derive_batch after the slots are taken: stage, derive on the device, copy the material back, make the handles
static int derive_batch_device(qpp_ctx *ctx, int suite, const uint8_t *secrets, const uint8_t *hp_in, size_t n,
                               uint32_t updates, const std::vector<uint32_t> &slots, qpp_key **out) {
    const size_t hl = suite_hash_len(suite), kl = suite_key_len(suite), mb = key_material_bytes();
    // key stage: secrets | hp_in | slots | material
    const size_t o_hp = n * hl, o_slot = o_hp + (hp_in ? n * kl : 0), o_mat = (o_slot + 4 * n + 15) & ~size_t(15);
    const size_t total = o_mat + n * mb;
    KStage *ks = nullptr;
    RC_TRY(take_kstage(ctx, total, &ks));
    uint8_t *h = ks->h, *d = ks->d;
    // the pinned stage holds secrets from here on: any exit below leaves them to the next take_kstage to zeroize
    ks->pending = total;
    memcpy(h, secrets, n * hl);
    if (hp_in) memcpy(h + o_hp, hp_in, n * kl);
    memcpy(h + o_slot, slots.data(), 4 * n);
    hipStream_t s = ctx->kstream;
    HIP_TRY(ctx, hipMemcpyAsync(d, h, o_slot + 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_key_derive(ctx->d_keys, (const uint32_t *)(d + o_slot), (uint32_t)n, suite, d,
                                   hp_in ? d + o_hp : nullptr, updates, d + o_mat, ctx->fips ? 1u : 0u, ctx->pow, s));
    HIP_TRY(ctx, hipMemcpyAsync(h + o_mat, d + o_mat, n * mb, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemsetAsync(d, 0, total, s));
    HIP_TRY(ctx, hipEventRecord(ctx->keys_ready, s));
    ctx->key_gen++;
    RC_TRY(release_kstage(ctx, ks, total));  // (zeroized below as well; an error exit in between leaves it pending)
    HIP_TRY(ctx, hipStreamSynchronize(s));  // the material comes back to the host handles
    const uint32_t nr = suite == QPP_SUITE_TLS_AES_128_GCM_SHA256 ? 10 : suite == QPP_SUITE_TLS_AES_256_GCM_SHA384 ? 14 : 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *m = h + o_mat + i * mb;
        qpp_key *k = new qpp_key();
        k->ctx = ctx;
        k->suite = suite;
        k->slot = slots[i];
        k->has_secret = true;
        memcpy(k->secret, m, hl);
        memcpy(k->key, m + 48, kl);
        memcpy(k->iv, m + 80, 12);
        memcpy(k->hp, m + 96, kl);
        // host mirror: what the host needs (suite, rounds, liveness); the record itself was written on the device
        DevKey &r = ctx->h_keys[slots[i]];
        memset(&r, 0, sizeof r);
        r.suite = (uint32_t)suite;
        r.nr = r.hp_nr = nr;
        r.live = 1;
        r.fips = ctx->fips && is_aes(suite) ? 1u : 0u;  // as key_derive_kernel sets it on the device
        ctx->fips_live += r.fips;
        ctx->live_slot_xor ^= slots[i];
        out[i] = k;
    }
    ctx->live_by_suite[suite] += (uint32_t)n;
    secure_zero(h, total);
    return QPP_OK;
}

// n secrets (n * hash_len, host) [+ header keys hp_in, n * key_len, host] -> n device-derived keys in fresh or
// recycled slots.  updates x "quic ku" on each; material copied back for the host handles.
static int derive_batch(qpp_ctx *ctx, int suite, const uint8_t *secrets, const uint8_t *hp_in, size_t n,
                        uint32_t updates, qpp_key **out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(flush_keys(ctx));  // pending host records first
    // (The records that flush just queued are copied from its key stage asynchronously; the derivation takes the
    // OTHER stage -- take_kstage -- so it neither waits for that copy nor overwrites the records: overwriting them was
    // found by tests/test_gpu_fuzz.py, a key created just before a batched update installed from the secrets written
    // over its record.)
    std::vector<uint32_t> slots;
    slots.reserve(n);
    // a failure after slots were taken gives them back through retirement (the device may have written their records)
    auto give_back = [&](int rc) {
        for (uint32_t s : slots) retire_slot(ctx, s);
        return rc;
    };
    for (size_t i = 0; i < n; i++) {
        uint32_t s = 0;
        if (int rc = alloc_slot(ctx, &s)) return give_back(rc);
        slots.push_back(s);
    }
    if (int rc = derive_batch_device(ctx, suite, secrets, hp_in, n, updates, slots, out)) return give_back(rc);
    return QPP_OK;
}

}  // namespace qpp

extern "C" {

int qpp_ctx_key_slots(qpp_ctx *ctx, uint32_t *capacity, uint32_t *high_water, uint32_t *retired) {
    if (!ctx) return QPP_INTERNAL_ERROR;
    if (capacity) *capacity = ctx->key_cap;
    if (high_water) *high_water = ctx->next_slot;
    if (retired) *retired = ctx->retired_slots + (uint32_t)ctx->retire_pending.size();
    return QPP_OK;
}

// ---------------------------------------------------------------- keys

int qpp_key_new(qpp_ctx *ctx, int suite, const uint8_t *secret, size_t secret_len, qpp_key **out) {
    if (!ctx || !out || !secret) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    if (secret_len != suite_hash_len(suite)) return QPP_INTERNAL_ERROR;
    qpp_key *k = new qpp_key();
    k->ctx = ctx;
    k->suite = suite;
    k->has_secret = true;
    memcpy(k->secret, secret, secret_len);
    derive(k);
    int rc = install(k);
    if (rc) { secure_zero(k, sizeof *k); delete k; return rc; }
    *out = k;
    return QPP_OK;
}

int qpp_key_new_pair(qpp_ctx *ctx, int suite, const uint8_t *secret, size_t secret_len, qpp_key **key,
                     qpp_header_key **header_key) {
    if (!key || !header_key) return QPP_INTERNAL_ERROR;
    *header_key = nullptr;
    RC_TRY(qpp_key_new(ctx, suite, secret, secret_len, key));
    int rc = qpp_header_key_new(ctx, suite, secret, secret_len, header_key);
    if (rc) { qpp_key_free(*key); *key = nullptr; }
    return rc;
}

int qpp_key_new_batch(qpp_ctx *ctx, int suite, const uint8_t *secrets, size_t n, uint32_t updates, qpp_key **out) {
    if (!ctx || !out || (n && !secrets)) return QPP_INTERNAL_ERROR;
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    if (n > (1u << 24)) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    return derive_batch(ctx, suite, secrets, nullptr, n, updates, out);
}

int qpp_key_update_batch(qpp_key *const *keys, size_t n, qpp_key **out) {
    if (!out || (n && !keys)) return QPP_INTERNAL_ERROR;
    if (!n) return QPP_OK;
    if (n > (1u << 24)) return QPP_INTERNAL_ERROR;
    for (size_t i = 0; i < n; i++) out[i] = nullptr;  // the caller's array may be uninitialised
    qpp_ctx *ctx = keys[0] ? keys[0]->ctx : nullptr;
    if (!ctx) return QPP_INTERNAL_ERROR;
    for (size_t i = 0; i < n; i++)
        if (!keys[i] || keys[i]->ctx != ctx || !keys[i]->has_secret) return QPP_INTERNAL_ERROR;
    // one device pass per suite present, each key's secret through one "quic ku" step, its header key kept
    std::vector<uint8_t> sec, hp;
    std::vector<size_t> idx;
    std::vector<qpp_key *> made;
    for (int suite = 1; suite <= 3; suite++) {
        idx.clear();
        for (size_t i = 0; i < n; i++)
            if (keys[i]->suite == suite) idx.push_back(i);
        if (idx.empty()) continue;
        const size_t hl = suite_hash_len(suite), kl = suite_key_len(suite);
        sec.resize(idx.size() * hl);
        hp.resize(idx.size() * kl);
        for (size_t j = 0; j < idx.size(); j++) {
            memcpy(sec.data() + j * hl, keys[idx[j]]->secret, hl);
            memcpy(hp.data() + j * kl, keys[idx[j]]->hp, kl);
        }
        made.resize(idx.size());
        int rc = derive_batch(ctx, suite, sec.data(), hp.data(), idx.size(), 1, made.data());
        secure_zero(sec.data(), sec.size());
        secure_zero(hp.data(), hp.size());
        if (rc) {
            for (size_t i = 0; i < n; i++)
                if (out[i]) { qpp_key_free(out[i]); out[i] = nullptr; }
            return rc;
        }
        for (size_t j = 0; j < idx.size(); j++) out[idx[j]] = made[j];
    }
    return QPP_OK;
}

int qpp_key_new_raw(qpp_ctx *ctx, int suite, const uint8_t *key, size_t key_len, const uint8_t iv[12],
                    const uint8_t *hp, size_t hp_len, qpp_key **out) {
    if (!ctx || !out || !key || !iv || !hp) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    if (key_len != suite_key_len(suite) || hp_len != suite_key_len(suite)) return QPP_INTERNAL_ERROR;
    qpp_key *k = new qpp_key();
    k->ctx = ctx;
    k->suite = suite;
    memcpy(k->key, key, key_len);
    memcpy(k->iv, iv, 12);
    memcpy(k->hp, hp, hp_len);
    int rc = install(k);
    if (rc) { secure_zero(k, sizeof *k); delete k; return rc; }
    *out = k;
    return QPP_OK;
}

int qpp_key_update(const qpp_key *key, qpp_key **out) {
    if (!key || !out) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    if (!key->has_secret) return QPP_INTERNAL_ERROR;
    qpp_key *k = new qpp_key();
    k->ctx = key->ctx;
    k->suite = key->suite;
    k->has_secret = true;
    const size_t hl = suite_hash_len(key->suite);
    hkdf_expand_label(hl, key->secret, "quic ku", k->secret, hl);
    derive(k);
    memcpy(k->hp, key->hp, sizeof k->hp);  // RFC 9001 §6: the header protection key is not updated
    int rc = install(k);
    if (rc) { secure_zero(k, sizeof *k); delete k; return rc; }
    *out = k;
    return QPP_OK;
}

int qpp_key_fips(const qpp_key *key) {
    if (!key || !key->ctx || key->slot >= key->ctx->key_cap) return 0;
    return key->ctx->h_keys[key->slot].fips ? 1 : 0;
}

void qpp_key_free(qpp_key *key) {
    if (!key) return;
    qpp_ctx *ctx = key->ctx;
    if (ctx && key->slot < ctx->key_cap && ctx->h_keys[key->slot].live == 1) {
        ctx->live_by_suite[key->suite]--;
        ctx->live_slot_xor ^= key->slot;
        ctx->fips_live -= ctx->h_keys[key->slot].fips;
        retire_slot(ctx, key->slot);
    }
    secure_zero(key, sizeof *key);
    delete key;
}

void qpp_key_free_batch(qpp_key *const *keys, size_t n) {
    if (!keys) return;
    for (size_t i = 0; i < n; i++) qpp_key_free(keys[i]);  // retirements only collect; one flush before the next use
}

uint32_t qpp_key_slot(const qpp_key *key) { return key ? key->slot : UINT32_MAX; }
void qpp_key_slot_batch(const qpp_key *const *keys, size_t n, uint32_t *slots) {
    if (!keys || !slots) return;
    for (size_t i = 0; i < n; i++) slots[i] = keys[i] ? keys[i]->slot : UINT32_MAX;
}
int qpp_key_suite(const qpp_key *key) { return key ? key->suite : 0; }
size_t qpp_tag_len(const qpp_key *) { return 16; }
size_t qpp_sample_len(const qpp_key *) { return 16; }
uint64_t qpp_confidentiality_limit(const qpp_key *key) {
    // cipher_suite.rs:261,281,298 (RFC 9001 §6.6)
    return key && key->suite == QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256 ? (1ULL << 62) : (1ULL << 23);
}
uint64_t qpp_integrity_limit(const qpp_key *key) {
    // cipher_suite.rs:262,282,299
    return key && key->suite == QPP_SUITE_TLS_CHACHA20_POLY1305_SHA256 ? (1ULL << 36) : (1ULL << 52);
}

int qpp_key_material(const qpp_key *key, uint8_t *key_out, uint8_t iv_out[12], uint8_t *hp_out) {
    if (!key) return QPP_INTERNAL_ERROR;
    const size_t kl = suite_key_len(key->suite);
    if (key_out) memcpy(key_out, key->key, kl);
    if (iv_out) memcpy(iv_out, key->iv, 12);
    if (hp_out) memcpy(hp_out, key->hp, kl);
    return QPP_OK;
}

// ---------------------------------------------------------------- header keys (header_key.rs)

int qpp_header_key_new_raw(qpp_ctx *ctx, int suite, const uint8_t *hp, size_t hp_len, qpp_header_key **out) {
    if (!ctx || !out || !hp) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    if (hp_len != suite_key_len(suite)) return QPP_INTERNAL_ERROR;
    qpp_header_key *h = new qpp_header_key();
    h->ctx = ctx;
    h->suite = suite;
    memcpy(h->hp, hp, hp_len);
    int rc = install_header(h);
    if (rc) { secure_zero(h, sizeof *h); delete h; return rc; }
    *out = h;
    return QPP_OK;
}

int qpp_header_key_new(qpp_ctx *ctx, int suite, const uint8_t *secret, size_t secret_len, qpp_header_key **out) {
    // HeaderKey::new(secret, "quic hp", alg) (header_key.rs:33-49), as TLS_*::new makes it (cipher_suite.rs:85-103)
    if (!ctx || !out || !secret) return QPP_INTERNAL_ERROR;
    *out = nullptr;
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    if (secret_len != suite_hash_len(suite)) return QPP_INTERNAL_ERROR;
    uint8_t hp[32];
    const size_t kl = suite_key_len(suite);
    hkdf_expand_label(secret_len, secret, "quic hp", hp, kl);
    int rc = qpp_header_key_new_raw(ctx, suite, hp, kl, out);
    secure_zero(hp, sizeof hp);
    return rc;
}

void qpp_header_key_free(qpp_header_key *hk) {
    if (!hk) return;
    qpp_ctx *ctx = hk->ctx;
    if (ctx && hk->slot < ctx->key_cap && ctx->h_keys[hk->slot].live == 2) {
        ctx->hdr_live_by_suite[ctx->h_keys[hk->slot].suite & 3]--;
        retire_slot(ctx, hk->slot);
    }
    secure_zero(hk, sizeof *hk);
    delete hk;
}

uint32_t qpp_header_key_slot(const qpp_header_key *hk) { return hk ? hk->slot : UINT32_MAX; }
int qpp_header_key_suite(const qpp_header_key *hk) { return hk ? hk->suite : 0; }
size_t qpp_header_key_sample_len(const qpp_header_key *) { return 16; }

int qpp_initial_keys(qpp_ctx *ctx, int endpoint, const uint8_t *dcid, size_t dcid_len, qpp_key **sealer,
                     qpp_key **opener) {
    return qpp_initial_keys_pair(ctx, endpoint, dcid, dcid_len, sealer, opener, nullptr, nullptr);
}

int qpp_initial_keys_pair(qpp_ctx *ctx, int endpoint, const uint8_t *dcid, size_t dcid_len, qpp_key **sealer,
                          qpp_key **opener, qpp_header_key **header_sealer, qpp_header_key **header_opener) {
    // quic/s2n-quic-crypto/src/initial.rs:29-68 -> (InitialKey, InitialHeaderKey); salt quic/s2n-quic-core/src/crypto/initial.rs:29
    static const uint8_t salt[20] = {0x38, 0x76, 0x2c, 0xf7, 0xf5, 0x59, 0x34, 0xb3, 0x4d, 0x17,
                                     0x9a, 0xe6, 0xa4, 0xc8, 0x0c, 0xad, 0xcc, 0xbb, 0x7f, 0x0a};
    if (!ctx || !sealer || !opener || (!dcid && dcid_len)) return QPP_INTERNAL_ERROR;
    if (!header_sealer != !header_opener) return QPP_INTERNAL_ERROR;
    *sealer = *opener = nullptr;
    if (header_sealer) *header_sealer = *header_opener = nullptr;
    uint8_t prk[32], client[32], server[32];
    hkdf_extract(32, salt, sizeof salt, dcid, dcid_len, prk);
    hkdf_expand_label(32, prk, "client in", client, 32);
    hkdf_expand_label(32, prk, "server in", server, 32);
    const bool is_client = endpoint == QPP_ENDPOINT_CLIENT;
    const uint8_t *ss = is_client ? client : server, *os = is_client ? server : client;
    const int suite = QPP_SUITE_TLS_AES_128_GCM_SHA256;
    int rc = qpp_key_new(ctx, suite, ss, 32, sealer);
    if (!rc) rc = qpp_key_new(ctx, suite, os, 32, opener);
    if (!rc && header_sealer) rc = qpp_header_key_new(ctx, suite, ss, 32, header_sealer);
    if (!rc && header_opener) rc = qpp_header_key_new(ctx, suite, os, 32, header_opener);
    if (rc) {
        qpp_key_free(*sealer); qpp_key_free(*opener);
        *sealer = *opener = nullptr;
        if (header_sealer) {
            qpp_header_key_free(*header_sealer); qpp_header_key_free(*header_opener);
            *header_sealer = *header_opener = nullptr;
        }
    }
    secure_zero(prk, sizeof prk); secure_zero(client, sizeof client); secure_zero(server, sizeof server);
    return rc;
}

int qpp_dc_key_new(qpp_ctx *ctx, int suite, const uint8_t *key, size_t key_len, const uint8_t iv[12], qpp_key **out) {
    // awslc.rs:24-33,157-166: key + iv only; the unused header-key slot stays zero
    static const uint8_t no_hp[32] = {0};
    if (!valid_suite(suite)) return QPP_UNSUPPORTED;
    return qpp_key_new_raw(ctx, suite, key, key_len, iv, no_hp, suite_key_len(suite), out);
}

}  // extern "C"
