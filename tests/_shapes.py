"""The shape grid of the header-length and block-count tests (tests/test_shape_grid.py on the CPU checkers,
tests/test_gpu_shapes.py on the kernels): (aad_len, pt_len, pn_len) cases and the batch that carries them.

A packet is a = ceil(aad_len / 16) header blocks, c = ceil(pt_len / 16) payload blocks and the length block:
m = a + c + 1 GHASH / Poly1305 blocks.  What the values are for:

aad_len   64 | 65: a quad lane gets a second header block (quad.hip's product loop runs); 128 | 129: a third;
          1008 | 1009 and 1024 | 1025: a = 63 | 64 | 65, a whole 64-lane burst pass of header; 65535: the field's limit.
pt_len    240 | 256: the end of the quad kernel's 16-slot group 0 and its HEAD condition; 4064: the counter's low byte
          wraps (the quad kernel's counter page changes); 20 - pn_len: the early header-protection condition.
m         63 | 64 | 65, 127 | 128 | 129, 192: the burst kernels' pass count K = ceil(m / 64), the idle lane pad - 1 that
          computes E_K(J0) (none when m % 64 == 0), the lane (pad + a) % 64 that holds the HP sample, and the servers'
          two-wave form (m <= 128).
"""
import numpy as np

import qpp

AAD_LENS = [None, 15, 16, 17, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 127, 128, 129, 255, 256, 257, 1007, 1008,
            1009, 1023, 1024, 1025, 2047, 4096, 65535]  # None: the PN bytes alone (aad_len = pn_len)
PT_LENS = [0, 1, 4, 15, 16, 17, 20, 239, 240, 241, 255, 256, 257, 960, 961, 976, 977, 1200, 4063, 4064, 4065, 4080,
           4096, 65535]
PN_LENS = [1, 4]
BIG = 65535
BLOCK_A = [1, 5, 40, 64, 100]
BLOCK_M = [63, 64, 65, 127, 128, 129, 192]


def blocks(aad_len, pt_len):
    """(a, m) of a packet"""
    a = (aad_len + 15) // 16
    return a, a + (pt_len + 15) // 16 + 1


def hp_ok(case):
    """the header-protection sample fits (packet/encoding.rs:178-188 pads a payload to ensure it)"""
    return case[1] + case[2] >= 4


def cross_cases():
    """every aad_len x pt_len x pn_len below 64 KiB, header length outermost: 46 neighbours share an aad_len"""
    return [(pn if aad is None else aad, pt, pn)
            for aad in AAD_LENS if aad != BIG for pn in PN_LENS for pt in PT_LENS if pt != BIG]


def block_rows():
    """for each a, payloads that make m each of BLOCK_M: header and payload ending on a block boundary, and both one
    byte past the boundary before (the same block counts with 1-byte last blocks)"""
    out = []
    for a in BLOCK_A:
        for m in BLOCK_M:
            c = m - a - 1
            if c < 0:
                continue
            pn = 4 if (c == 0 or (a + m) % 2) else 1
            out.append((16 * a, 16 * c, pn))
            if c >= 1:
                out.append((16 * (a - 1) + 1, 16 * (c - 1) + 1, 5 - pn if a > 1 else 1))
    return out


def big_rows():
    """the 64 KiB rows: the longest header over a few payloads, the longest payload over a few headers, and both"""
    out = [(BIG, pt, 4 if i % 2 == 0 else 1) for i, pt in enumerate([0, 17, 1200, 4065])]
    out += [(aad, BIG, 1 if i % 2 == 0 else 4) for i, aad in enumerate([1, 16, 65, 129, 1009, 1025, 4096])]
    return out + [(BIG, BIG, 4)]


def hp_edge_rows():
    """pn_len 1 on both sides of the early-HP condition pt_len + pn_len >= 20 (pn_len 4 has 15 | 16 | 17 in the cross)
    and of the smallest payload that holds the sample, pt_len + pn_len >= 4"""
    return [(aad, pt, 1) for aad in (21, 65, 129, 1009) for pt in (2, 3, 18, 19)]


def grid_cases(hp=False):
    """the grid below 64 KiB: cross_cases() + block_rows() + hp_edge_rows(); hp: only the cases header protection can
    be applied to"""
    cases = cross_cases() + block_rows() + hp_edge_rows()
    return [c for c in cases if hp_ok(c)] if hp else cases


def build_batch(cases, key_slots, seed, shuffle=False):
    """(descs, arena) for a case list: packets in the list's order (shuffle: a seeded permutation of it, so that long
    and short headers share a wave), 0-8 random bytes between packets, 64 bytes of slack behind the last one (the
    kernels load whole 16-byte blocks), random bytes everywhere, random 62-bit packet numbers (every other one
    >= 2^32), key_idx a seeded choice among key_slots."""
    rng = np.random.default_rng(seed)
    n = len(cases)
    lens = np.asarray(cases, dtype=np.int64).reshape(n, 3)
    if shuffle:
        lens = lens[rng.permutation(n)]
    sizes = lens[:, 0] + lens[:, 1] + 16
    gaps = rng.integers(0, 9, n)
    offs = np.concatenate([[0], np.cumsum(sizes + gaps)[:-1]]).astype(np.int64)
    total = int(offs[-1] + sizes[-1] + 64)
    assert total < 1 << 32
    arena = rng.integers(0, 256, total, dtype=np.uint8)
    pn = rng.integers(0, 2**62, n, dtype=np.uint64)
    pn[0::2] |= np.uint64(1 << 32)
    pn[1::2] &= np.uint64((1 << 32) - 1)
    descs = np.zeros(n, dtype=qpp.PKT_DTYPE)
    descs["pn"] = pn
    descs["key_idx"] = np.asarray(key_slots, dtype=np.uint32)[rng.integers(0, len(key_slots), n)]
    descs["off"] = offs
    descs["aad_len"] = lens[:, 0]
    descs["pt_len"] = lens[:, 1]
    descs["pn_len"] = lens[:, 2]
    return descs, arena


def with_slots(descs, slots):
    """descs built over key indices 0..K-1, with the device slots of those keys in their place"""
    d = descs.copy()
    d["key_idx"] = np.asarray(slots, dtype=np.uint32)[descs["key_idx"].astype(np.int64)]
    return d
