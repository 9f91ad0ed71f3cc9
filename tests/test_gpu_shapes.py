"""Long headers and block-count edges (tests/_shapes.py) on every AEAD kernel path, on the GPU.

The parity suite is broad in payload length and key count and narrow in header length: no batch, receive, transmit-queue
or packet-server test sends more than 63 header bytes, so the AAD loops of the kernels past their first block per lane
(quad.hip quad_packet's product loop, the burst and server kernels' passes with a >= 64 header blocks, the per-lane and
per-wave loops of the other kernels) and the burst kernels' lane arithmetic at m = 63 | 64 | 65 ... blocks were reached
by chance or not at all.  Here every path seals and opens the grid with a fresh context per key set, so that each kernel
instance is reached on purpose (host.h suite_mask: AES-128 only, AES-256 only, both sizes; one live AES key: the
plan-less single launch).

Bar: bit-exact against OpenSSL (orc.fast_seal_batch; tests/test_shape_grid.py ties it to the restatement on the same
grid) -- arena, masks, status, every status entry written; the restatement where OpenSSL has no entry point (the receive
path, a protected packet).
"""
import functools

import numpy as np
import pytest

import _oracle as orc
import _shapes
import qpp

pytestmark = pytest.mark.gpu
HP = qpp.HP_MASK_OUT | qpp.HP_APPLY

KEYSETS = {"aes128x1": [1], "aes128x2": [1, 1], "aes256x1": [2], "aes256x2": [2, 2], "mixed": [1, 2, 3], "chacha": [3]}
# kernel path x key set: the AES paths over every set with an AES key (the mixed set's ChaCha20 packets take the burst
# or the lane ChaCha20 kernel with them), ChaCha20 alone both ways
COMBOS = [(p, k) for k in ("aes128x1", "aes128x2", "aes256x1", "aes256x2", "mixed") for p in ("burst", "quad", "wave")]
COMBOS += [("burst", "chacha"), ("lane", "chacha")]


def _configure(ctx, path):
    ctx.set_burst_max(1 << 30 if path == "burst" else 0)
    ctx.set_aes_kernel({"quad": qpp.AES_KERNEL_QUAD, "wave": qpp.AES_KERNEL_WAVE}.get(path, qpp.AES_KERNEL_AUTO))


@functools.lru_cache(maxsize=None)
def _secrets(keyset):
    rng = np.random.default_rng(sum(keyset.encode()) * 131 + len(keyset))
    return [(s, rng.integers(0, 256, qpp.HASH_LEN[s], dtype=np.uint8).tobytes()) for s in KEYSETS[keyset]]


@functools.lru_cache(maxsize=None)
def _materials(keyset):
    return [(s, *orc.derive(s, secret)) for s, secret in _secrets(keyset)]


def _make_keys(ctx, keyset):
    keys = [ctx.key(s, secret) for s, secret in _secrets(keyset)]
    for k, m in zip(keys, _materials(keyset)):
        assert (k.suite, *k.material()) == m
    return keys


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _sealed(keyset, which, shuffle, flags):
    """(descs over key indices, arena, OpenSSL's sealed arena, its masks): computed once, shared, read-only"""
    cases = _shapes.big_rows() if which == "big" else _shapes.grid_cases(hp=bool(flags))
    descs, arena = _shapes.build_batch(cases, range(len(KEYSETS[keyset])), 900 + len(keyset) + 2 * shuffle + (flags != 0),
                                       shuffle=shuffle)
    assert len(descs) == len(cases)
    want = arena.copy()
    masks = orc.fast_seal_batch(orc.make_keys(_materials(keyset)), descs, want, flags)
    return _ro(descs, arena, want, masks.copy())


@functools.lru_cache(maxsize=None)
def _tampered(keyset, which, shuffle):
    """the no-HP ciphertext with one packet in seven (of the 64 KiB rows: in three) tampered -- the last AAD byte, AAD
    byte 64 (when there is one), a ciphertext byte, a tag byte in turn -- and the arena an open must leave:
    DECRYPT_ERROR and a zeroed payload exactly on those, the plaintext back everywhere else, header and tag bytes as
    received"""
    descs, arena, sealed, _ = _sealed(keyset, which, shuffle, 0)
    n = len(descs)
    ct, want_st = sealed.copy(), np.zeros(n, dtype=np.int8)
    kinds = np.zeros(4, dtype=np.int64)
    for j, i in enumerate(range(3, n, 7) if which == "grid" else range(0, n, 3)):
        o, al, pl = int(descs[i]["off"]), int(descs[i]["aad_len"]), int(descs[i]["pt_len"])
        kind = j % 4
        if kind == 1 and al <= 64:
            kind = 0
        if kind == 2 and pl == 0:
            kind = 3
        pos = (o + al - 1, o + 64, o + al + (i * 7) % max(pl, 1), o + al + pl + i % 16)[kind]
        ct[pos] ^= np.uint8(1 << (i % 8))
        kinds[kind] += 1
        want_st[i] = qpp.DECRYPT_ERROR
    want = ct.copy()
    for i in range(n):
        o, al, pl = int(descs[i]["off"]), int(descs[i]["aad_len"]), int(descs[i]["pt_len"])
        want[o + al:o + al + pl] = 0 if want_st[i] else arena[o + al:o + al + pl]
    return _ro(ct, want, want_st) + (kinds,)


def _seal(ctx, descs, arena, flags):
    n = len(descs)
    bufs = d_desc, d_arena, d_mask, d_status = ctx.alloc(descs.nbytes), ctx.alloc(arena.nbytes), ctx.alloc(5 * n), ctx.alloc(n)
    d_desc.upload(descs)
    d_arena.upload(arena)
    d_status.upload(np.full(n, 0x55, dtype=np.int8))
    ctx.seal_batch(d_desc, n, d_arena, d_mask, d_status, flags)
    ctx.sync()
    out = d_arena.download(), d_mask.download(), d_status.download(dtype=np.int8)
    for b in bufs:
        b.free()
    return out


def _open(ctx, descs, arena):
    n = len(descs)
    bufs = d_desc, d_arena, d_status = ctx.alloc(descs.nbytes), ctx.alloc(arena.nbytes), ctx.alloc(n)
    d_desc.upload(descs)
    d_arena.upload(arena)
    d_status.upload(np.full(n, 0x55, dtype=np.int8))
    ctx.open_batch(d_desc, n, d_arena, d_status)
    ctx.sync()
    out = d_arena.download(), d_status.download(dtype=np.int8)
    for b in bufs:
        b.free()
    return out


def _same_arena(got, want, descs, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(descs["off"].astype(np.int64), bad[0], side="right")) - 1
        d = descs[i]
        raise AssertionError(f"{what}: arena differs first at byte {int(bad[0])}, packet {i} (aad_len {int(d['aad_len'])}, "
                             f"pt_len {int(d['pt_len'])}, pn_len {int(d['pn_len'])}, byte {int(bad[0]) - int(d['off'])} "
                             f"of it); {bad.size} bytes differ")


def _same_status(got, want, descs, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        d = descs[int(bad[0])]
        raise AssertionError(f"{what}: status of packet {int(bad[0])} is {int(got[bad[0]])}, not {int(want[bad[0]])} "
                             f"(aad_len {int(d['aad_len'])}, pt_len {int(d['pt_len'])}); {bad.size} differ")


def _seal_open(path, keyset, which, shuffle):
    ctx = qpp.Context(0)
    keys = []
    try:
        _configure(ctx, path)
        keys = _make_keys(ctx, keyset)
        slots = [k.slot for k in keys]
        for flags in (0, HP):
            descs_i, arena, want, want_masks = _sealed(keyset, which, shuffle, flags)
            descs = _shapes.with_slots(descs_i, slots)
            got, masks, st = _seal(ctx, descs, arena, flags)
            _same_status(st, np.zeros(len(descs), dtype=np.int8), descs, f"seal flags {flags}")
            _same_arena(got, want, descs, f"seal flags {flags}")
            if flags:
                bad = np.flatnonzero(masks != want_masks)
                assert bad.size == 0, f"HP mask of packet {int(bad[0]) // 5} differs: {descs[int(bad[0]) // 5]}"
        descs = _shapes.with_slots(_sealed(keyset, which, shuffle, 0)[0], slots)
        ct, want, want_st, kinds = _tampered(keyset, which, shuffle)
        if which == "grid":  # every tamper position is used, AAD byte 64 among them
            assert (kinds >= 20).all(), kinds
        else:
            assert (kinds >= 1).all(), kinds
        got, st = _open(ctx, descs, ct)
        _same_status(st, want_st, descs, "open")
        _same_arena(got, want, descs, "open")
    finally:
        for k in keys:
            k.free()
        ctx.close()


# ------------------------------------------------------------------ a. batch seal and open

@pytest.mark.parametrize("order", ["given", "shuffled"])
@pytest.mark.parametrize("path,keyset", COMBOS, ids=[f"{p}-{k}" for p, k in COMBOS])
def test_batch_seal_open_grid(path, keyset, order):
    """the grid below 64 KiB: as given (the 16 packets of a quad-kernel wave alike: its wave-uniform loop shape at each
    header length) and shuffled (long and short headers in one wave)"""
    _seal_open(path, keyset, "grid", order == "shuffled")


BIG_COMBOS = [("burst", "aes128x1"), ("quad", "aes128x1"), ("wave", "aes128x1"), ("burst", "aes256x1"),
              ("quad", "aes256x1"), ("wave", "aes256x1"), ("burst", "chacha"), ("lane", "chacha")]


@pytest.mark.parametrize("path,keyset", BIG_COMBOS, ids=[f"{p}-{k}" for p, k in BIG_COMBOS])
def test_batch_seal_open_64k_rows(path, keyset):
    """aad_len and pt_len at the fields' limit, 65535 (one key set per suite, in the given order)"""
    _seal_open(path, keyset, "big", False)


# ------------------------------------------------------------------ b. receive path

RX_PAYLOADS = [None, 17, 20, 257, 1200]  # None: the shortest payload that holds the sample, 4 - pn_len


@functools.lru_cache(maxsize=None)
def _rx_batch(suite):
    """long-header packets with header lengths of the grid up to 4096 B as a peer sends them (orc.protect_packet), the
    case list repeated with fresh packet numbers to 2048+ packets; some tags, some header bytes tampered, some packets
    too short for the sample.  Returns (key material, rx over key index 0, arena, the restatement's arena,
    descriptors and statuses)."""
    rng = np.random.default_rng(3100 + suite)
    mat = (suite, *orc.derive(suite, rng.integers(0, 256, qpp.HASH_LEN[suite], dtype=np.uint8).tobytes()))
    cases = [(aad - pn, pt, pn) for j, aad in enumerate(a for a in _shapes.AAD_LENS if a and a <= 4096)
             for pn in _shapes.PN_LENS for pt in RX_PAYLOADS if aad - pn >= 1]
    reps = -(-2048 // len(cases))
    chunks, rx, off = [], [], 0
    n_hdr = n_tag = n_short = 0
    for i, (hl, pt, pn_len) in enumerate(cases * reps):
        pt = 4 - pn_len if pt is None else pt
        pn = int(rng.integers(1000, 2**62 - 1))
        largest = pn - 1 - int(rng.integers(0, 100))  # (within the window of a 1-byte encoding)
        first = 0xc0 | (int(rng.integers(0, 4)) << 4) | (pn_len - 1)
        header = bytes([first]) + rng.integers(0, 256, hl - 1, dtype=np.uint8).tobytes()
        payload = rng.integers(0, 256, pt, dtype=np.uint8).tobytes()
        rc, pkt = orc.protect_packet(*mat, pn, header, pn_len, payload)
        assert rc == 0
        pkt = bytearray(pkt)
        length = len(pkt)
        if i % 11 == 3:
            pkt[-1 - i % 16] ^= 0x20  # a tag byte
            n_tag += 1
        elif i % 11 == 7:  # a header byte: the last, byte 64, byte 1 or the first byte's packet-type bits in turn
            pos = (hl - 1, 64 if hl > 64 else hl // 2, min(1, hl - 1), 0)[(i // 11) % 4]
            pkt[pos] ^= 0x10
            n_hdr += 1
        elif i % 13 == 5:
            length = hl + 19  # no room for the 16-byte sample at header_len + 4
            pkt = pkt[:length]
            n_short += 1
        chunks.append(bytes(pkt) + bytes(int(rng.integers(0, 7))))
        rx.append((largest, (0, 0), off, hl, length))
        off += len(chunks[-1])
    assert len(rx) >= 2048 and min(n_hdr, n_tag, n_short) >= 50
    rx = np.array(rx, dtype=qpp.RX_DTYPE)
    arena = np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy()
    want_arena = arena.copy()
    want_out, want_st = orc.unprotect_open_batch(orc.make_keys([mat]), rx, want_arena)
    want_st = np.array(want_st, dtype=np.int8)
    assert (want_st == qpp.DECRYPT_ERROR).sum() == n_hdr + n_tag and (want_st == qpp.DECODE_ERROR).sum() == n_short
    assert (want_st == qpp.OK).sum() > len(rx) // 2
    return (mat,) + _ro(rx, arena, want_arena, want_out, want_st)


def _rx_run(ctx, rx, arena):
    n = len(rx)
    bufs = d_rx, d_arena, d_out, d_status = (ctx.alloc(rx.nbytes), ctx.alloc(arena.nbytes),
                                             ctx.alloc(n * qpp.PKT_DTYPE.itemsize), ctx.alloc(n))
    d_rx.upload(rx)
    d_arena.upload(arena)
    d_out.upload(np.full(n * qpp.PKT_DTYPE.itemsize, 0x55, dtype=np.uint8))
    d_status.upload(np.full(n, 0x55, dtype=np.int8))
    ctx.unprotect_open_batch(d_rx, n, d_arena, d_out, d_status)
    ctx.sync()
    out = d_arena.download(), d_out.download(dtype=qpp.PKT_DTYPE), d_status.download(dtype=np.int8)
    for b in bufs:
        b.free()
    return out


@pytest.mark.parametrize("suite", [1, 2, 3], ids=["aes128", "aes256", "chacha"])
def test_receive_long_headers(suite, monkeypatch):
    """qpp_unprotect_open_batch over long headers: the fused launch (one live AES key: quad.hip's receive kernel, several
    workgroup slices; ChaCha20 alone: the lane kernel's one launch) and the multi-launch path equal each other and the
    restatement -- statuses, descriptors out, arena"""
    mat, rx0, arena, want_arena, want_out, want_st = _rx_batch(suite)
    ctx = qpp.Context(0)
    k = None
    try:
        ctx.set_burst_max(0)
        ctx.set_aes_kernel(qpp.AES_KERNEL_QUAD)
        k = ctx.raw_key(suite, *mat[1:])
        rx = rx0.copy()
        rx["key_idx"][:] = k.slot
        res = {}
        for fused in (True, False):
            monkeypatch.setenv("QPP_RX_FUSED", "1" if fused else "0")
            a, o, st = _rx_run(ctx, rx, arena)
            what = "fused" if fused else "multi-launch"
            bad = np.flatnonzero(st != want_st)
            assert bad.size == 0, f"{what}: status of packet {int(bad[0])} is {int(st[bad[0]])}, not " \
                                  f"{int(want_st[bad[0]])}: {rx[int(bad[0])]}; {bad.size} differ"
            bad = np.flatnonzero(a != want_arena)
            assert bad.size == 0, f"{what}: arena differs first at byte {int(bad[0])}, packet " \
                f"{int(np.searchsorted(rx['off'].astype(np.int64), bad[0], side='right')) - 1}; {bad.size} bytes differ"
            for f in ("pn", "aad_len", "pt_len", "pn_len", "flags", "off"):
                assert (o[f] == want_out[f]).all(), (what, f)
            assert (o["key_idx"] == k.slot).all()
            res[fused] = (a, o, st)
        assert ctx.rx_timeouts() == 0
        assert (res[True][0] == res[False][0]).all() and (res[True][2] == res[False][2]).all()
        assert (res[True][1].view(np.uint8) == res[False][1].view(np.uint8)).all()
    finally:
        if k:
            k.free()
        ctx.close()


# ------------------------------------------------------------------ c. transmit queue

@functools.lru_cache(maxsize=None)
def _tx_cases():
    """the block-count rows and long-header rows (headers up to 1025 B), as (header_len, pt_len, pn_len)"""
    rows = [c for c in _shapes.block_rows() if _shapes.hp_ok(c) and c[0] > c[2]]
    for j, aad in enumerate(a for a in _shapes.AAD_LENS if a and a <= 1025):
        for i, pt in enumerate((None, 20, 241, 1200)):
            pn = _shapes.PN_LENS[(i + j) % 2]
            rows.append((aad, 4 - pn if pt is None else pt, pn))
    assert {_shapes.blocks(c[0], c[1])[1] for c in rows} >= set(_shapes.BLOCK_M)
    return [(aad - pn, pt, pn) for aad, pt, pn in rows]


@pytest.mark.parametrize("mode", ["zero_copy-burst", "zero_copy-quad", "dma-burst", "dma-quad", "persistent"])
def test_txq_long_headers_and_block_counts(mode, monkeypatch):
    """TxQueue.flush: every case under a key of each suite (the persistent queue: the AES suites), each packet equal to
    crypto::encrypt + crypto::protect of the restatement; the persistent queue's flush is the server's, not launched"""
    flush, _, path = mode.partition("-")
    monkeypatch.setenv("QPP_TXQ_ZC_MAX", "0" if flush == "dma" else "1024")
    monkeypatch.setenv("QPP_TXQ_SERVER_IDLE_MS", "4000")
    rng = np.random.default_rng(3200)
    ctx = qpp.Context(0)
    keys, q = [], None
    try:
        if path:
            _configure(ctx, path)
        suites = (1, 2) if flush == "persistent" else (1, 2, 3)
        keys = [ctx.key(s, rng.integers(0, 256, qpp.HASH_LEN[s], dtype=np.uint8).tobytes()) for s in suites]
        cases = _tx_cases()
        n = len(cases) * len(keys)
        assert n <= 1024
        q = qpp.TxQueue(ctx, 1 << 20, 1024, persistent=flush == "persistent")
        want, off = [], 0
        for i, (hl, pt, pn_len) in enumerate(cases):
            for k in keys:
                pn = int(rng.integers(0, 2**62))
                header = bytes([0xc0 | (pn_len - 1)]) + rng.integers(0, 256, hl - 1, dtype=np.uint8).tobytes()
                payload = rng.integers(0, 256, pt, dtype=np.uint8).tobytes()
                pkt = header + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big") + payload
                q.ring[off:off + len(pkt)] = np.frombuffer(pkt, dtype=np.uint8)
                q.push(k, pn, off, hl, pn_len, pt)
                rc, protected = orc.protect_packet(k.suite, *k.material(), pn, header, pn_len, payload)
                assert rc == 0
                want.append((off, protected, (hl, pt, pn_len, k.suite)))
                off += len(protected) + int(rng.integers(0, 5))
        assert off + 64 <= 1 << 20 and q.pending() == n
        q.flush()
        assert q.pending() == 0
        for o, p, case in want:
            assert q.ring[o:o + len(p)].tobytes() == p, case
        if flush == "persistent":
            assert q.info()[:2] == (1, 0) and q.server_refused() == 0
    finally:
        if q:
            q.close()
        for k in keys:
            k.free()
        ctx.close()


# ------------------------------------------------------------------ d. per-packet face

PKT_RING = 16384  # packet.cpp kPktRing: header + payload + tag up to this go through the packet server


@functools.lru_cache(maxsize=None)
def _pkt_cases():
    rows = [(c[0], c[1]) for c in _shapes.block_rows()]
    rows += [(hl, pt) for hl in (64, 65, 129, 1009, 4096) for pt in (0, 17, 241, 1200)]
    rows += [(hl, total - hl - 16) for total in (PKT_RING - 1, PKT_RING, PKT_RING + 1) for hl in (21, 4096)]
    return rows


@pytest.mark.parametrize("suite", [1, 2, 3], ids=["aes128", "aes256", "chacha"])
def test_per_packet_long_headers_and_block_counts(suite):
    """Key.encrypt / Key.decrypt with the packet server on and off: both equal the restatement's seal and each other,
    an AAD-tampered open is refused, and the server took exactly the calls that fit its ring"""
    rng = np.random.default_rng(3300 + suite)
    on, off = qpp.Context(0), qpp.Context(0)
    try:
        off.set_packet_server(False)
        secret = rng.integers(0, 256, qpp.HASH_LEN[suite], dtype=np.uint8).tobytes()
        a, b = on.key(suite, secret), off.key(suite, secret)
        kk, iv, _ = a.material()
        served = 0
        for hl, pt in _pkt_cases():
            pn = int(rng.integers(0, 2**62))
            header = rng.integers(0, 256, hl, dtype=np.uint8).tobytes()
            payload = rng.integers(0, 256, pt, dtype=np.uint8).tobytes()
            want = b"".join(orc.seal(suite, kk, orc.nonce(iv, pn), header, payload))
            bad = bytearray(header)
            bad[64 if hl > 64 and pt % 2 else hl - 1] ^= 0x04
            for k in (a, b):
                assert k.encrypt(pn, header, payload) == want, (hl, pt)
                assert k.decrypt(pn, header, want) == payload, (hl, pt)
                with pytest.raises(qpp.DecryptError):
                    k.decrypt(pn, bytes(bad), want)
            served += 3 * (hl + pt + 16 <= PKT_RING)
        calls, starts = on.packet_server_info()
        assert calls == served and starts >= 1
        assert served == 3 * (len(_pkt_cases()) - 2)  # (the two 16385-byte totals are launched)
        assert off.packet_server_info() == (0, 0)
        a.free()
        b.free()
    finally:
        on.close()
        off.close()
