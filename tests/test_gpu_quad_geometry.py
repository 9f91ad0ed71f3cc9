"""The AES-128 quad seal / open pair at its own workgroup geometry (quad.hip QPP_QUAD_WG128: 1024 threads, a pass of 256
packets, four waves per SIMD) at the packet counts where a pass of that width can go wrong, and the build-time guard
that holds the pair to that occupancy.

quad_slices gives workgroup b the packets [b P, (b + 1) P), P = (ceil(n / grid) + 15) & ~15, and walks them 256 at a
time, a quad (4 lanes) per packet: n = 1 is one quad; 15 | 16 | 17 one wave and its edge; 255 | 256 | 257 one pass and
its edge on a single workgroup's worth of waves; 4093 gives every workgroup of a 256-CU grid one wave (the last one 13
packets) and 3001 under two keys goes through the plan (perm, key segments).  The payload lengths are the group loop's
edges: 1 B (the last group only; the header-protection sample runs into the tag), 19 B, 239 | 240 | 241 B (the head
path's 15-block condition), 300 B (a last group of one block per lane), 1200 B, 4100 B (past 4080 B: the counter page
is rebuilt inside a group), and all of them mixed within a wave.  Header lengths 21 B and 50 B (four blocks: every lane
of the quad holds one).

Bar: bit-exact against OpenSSL (orc.fast_seal_batch) -- every packet's bytes, every header-protection mask, every
status; the open returns the plaintext byte for byte, DECRYPT_ERROR and a zeroed payload exactly on the tampered tags.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import _shapes
import qpp

HP = qpp.HP_MASK_OUT | qpp.HP_APPLY
MIX = [1, 15, 19, 239, 240, 241, 300, 1200, 4100]
# id: (suites of the keys, packets, header bytes, payload lengths -- cycled, or drawn per packet for "mixed")
CASES = {
    "n1-1200": ([1], 1, 21, [1200]),
    "n15-1": ([1], 15, 21, [1]),
    "n16-19": ([1], 16, 21, [19]),
    "n17-239": ([1], 17, 50, [239]),
    "n255-240": ([1], 255, 21, [240]),
    "n256-241": ([1], 256, 50, [241]),
    "n257-300": ([1], 257, 21, [300]),
    "n16-4100": ([1], 16, 50, [4100]),
    "n256-1200": ([1], 256, 21, [1200]),
    "n4093-mixed": ([1], 4093, 21, None),
    "n3001-1200-2keys": ([1, 1], 3001, 21, [1200]),
    "n64-1200-aes256": ([2], 64, 21, [1200]),
}


@functools.lru_cache(maxsize=None)
def _materials(case):
    suites = CASES[case][0]
    rng = np.random.default_rng(7100 + sum(case.encode()))
    return [(s, *orc.derive(s, rng.integers(0, 256, qpp.HASH_LEN[s], dtype=np.uint8).tobytes())) for s in suites]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _batch(case):
    """(descs over key indices, arena): computed once, read-only"""
    suites, n, aad, pts = CASES[case]
    rng = np.random.default_rng(7200 + sum(case.encode()))
    rows = []
    for i in range(n):
        pt = int(rng.choice(MIX)) if pts is None else pts[i % len(pts)]
        pn_len = 1 + i % 4
        if pt + pn_len < 4:  # the sample must fit (packet/encoding.rs:178-188)
            pn_len = 3 + i % 2
        rows.append((aad, pt, pn_len))
    return _ro(*_shapes.build_batch(rows, range(len(suites)), 7300 + n))


@functools.lru_cache(maxsize=None)
def _sealed(case, flags):
    """(OpenSSL's sealed arena, its masks)"""
    descs, arena = _batch(case)
    want = arena.copy()
    masks = orc.fast_seal_batch(orc.make_keys(_materials(case)), descs, want, flags)
    return _ro(want, masks.copy())


@functools.lru_cache(maxsize=None)
def _tampered(case):
    """the unprotected ciphertext with a handful of tag bytes flipped (the first, the last and a few packets between),
    the arena an open must leave and its statuses"""
    descs, arena = _batch(case)
    n = len(descs)
    ct, want_st = _sealed(case, 0)[0].copy(), np.zeros(n, dtype=np.int8)
    for i in sorted({0, n - 1, n // 2, n // 3, (2 * n) // 3, min(n - 1, 255), min(n - 1, 256)}):
        o, al, pl = int(descs[i]["off"]), int(descs[i]["aad_len"]), int(descs[i]["pt_len"])
        ct[o + al + pl + i % 16] ^= np.uint8(1 << (i % 8))
        want_st[i] = qpp.DECRYPT_ERROR
    want = ct.copy()
    for i in range(n):
        o, al, pl = int(descs[i]["off"]), int(descs[i]["aad_len"]), int(descs[i]["pt_len"])
        want[o + al:o + al + pl] = 0 if want_st[i] else arena[o + al:o + al + pl]
    return _ro(ct, want, want_st)


def _first_bad(got, want, descs, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(descs["off"].astype(np.int64), bad[0], side="right")) - 1
        d = descs[i]
        raise AssertionError(f"{what}: arena differs first at byte {int(bad[0])}, packet {i} of {len(descs)} (aad_len "
                             f"{int(d['aad_len'])}, pt_len {int(d['pt_len'])}, pn_len {int(d['pn_len'])}, byte "
                             f"{int(bad[0]) - int(d['off'])} of it); {bad.size} bytes differ")


def _run(ctx, seal, descs, arena, flags=0):
    n = len(descs)
    bufs = d_desc, d_arena, d_mask, d_status = ctx.alloc(descs.nbytes), ctx.alloc(arena.nbytes), ctx.alloc(5 * n), ctx.alloc(n)
    d_desc.upload(descs)
    d_arena.upload(arena)
    d_status.upload(np.full(n, 0x55, dtype=np.int8))
    if seal:
        ctx.seal_batch(d_desc, n, d_arena, d_mask, d_status, flags)
    else:
        ctx.open_batch(d_desc, n, d_arena, d_status)
    ctx.sync()
    out = d_arena.download(), d_mask.download(), d_status.download(dtype=np.int8)
    for b in bufs:
        b.free()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_quad_seal_open_at_pass_edges(case):
    ctx = qpp.Context(0)
    keys = []
    try:
        ctx.set_burst_max(0)  # the quad path at every size
        ctx.set_aes_kernel(qpp.AES_KERNEL_QUAD)
        keys = [ctx.raw_key(*m) for m in _materials(case)]
        descs_i, arena = _batch(case)
        descs = _shapes.with_slots(descs_i, [k.slot for k in keys])
        ok = np.zeros(len(descs), dtype=np.int8)
        for flags in (0, HP):
            want, want_masks = _sealed(case, flags)
            got, masks, st = _run(ctx, True, descs, arena, flags)
            assert (st == ok).all(), f"seal flags {flags}: status of packet {int(np.flatnonzero(st != ok)[0])}"
            _first_bad(got, want, descs, f"seal flags {flags}")
            if flags:
                bad = np.flatnonzero(masks != want_masks)
                assert bad.size == 0, f"HP mask of packet {int(bad[0]) // 5} differs: {descs[int(bad[0]) // 5]}"
        ct, want, want_st = _tampered(case)
        got, _, st = _run(ctx, False, descs, ct)
        bad = np.flatnonzero(st != want_st)
        assert bad.size == 0, f"open: status of packet {int(bad[0])} is {int(st[bad[0]])}, not {int(want_st[bad[0]])}"
        _first_bad(got, want, descs, "open")
    finally:
        for k in keys:
            k.free()
        ctx.close()


# ------------------------------------------------------------------ the build-time guard (no GPU)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "s2n-quic_amd", "csrc")
SEAL128 = "_ZN3qpp12_GLOBAL__N_119aes_gcm_quad_kernelILb1ELi10EEEvPKNS_6DevKeyE"
OPEN128 = "_ZN3qpp12_GLOBAL__N_119aes_gcm_quad_kernelILb0ELi10EEEvPKNS_6DevKeyE"
SEAL256 = "_ZN3qpp12_GLOBAL__N_119aes_gcm_quad_kernelILb1ELi14EEEvPKNS_6DevKeyE"


def _res(kernels):
    """a resource report in the compiler's remark format: {name: (scratch bytes per lane, waves per SIMD)}"""
    out = []
    for name, (scratch, occ) in kernels.items():
        for field in (f"Function Name: {name}", "    VGPRs: 128", f"    ScratchSize [bytes/lane]: {scratch}",
                      f"    Occupancy [waves/SIMD]: {occ}", "    LDS Size [bytes/block]: 0"):
            out.append(f"quad.hip:1:0: remark: {field} [-Rpass-analysis=kernel-resource-usage]")
    return "\n".join(out) + "\n"


def _guard(*paths):
    return subprocess.run([sys.executable, os.path.join(CSRC, "check_resources.py"), *paths], capture_output=True, text=True)


@pytest.mark.parametrize("seal,open_,ok", [((32, 4), (32, 4), True), ((0, 4), (16, 4), True), ((32, 3), (32, 4), False),
                                          ((32, 4), (32, 3), False), ((48, 4), (32, 4), False), ((32, 4), (36, 4), False)])
def test_resource_guard_rules(tmp_path, seal, open_, ok):
    """the AES-128 pair must report 4 waves per SIMD and at most 32 B/lane of scratch; the AES-256 instances stay at 3"""
    path = tmp_path / "quad.res"
    path.write_text(_res({SEAL128: seal, OPEN128: open_, SEAL256: (0, 3)}))
    r = _guard(str(path))
    assert (r.returncode == 0) == ok, r.stderr
    if not ok:
        assert "aes_gcm_quad_kernel" in r.stderr


def test_resource_guard_needs_the_pair(tmp_path):
    """a quad.res without the pair's remarks (a renamed kernel, a report cut short) does not pass by saying nothing"""
    path = tmp_path / "quad.res"
    path.write_text(_res({SEAL128: (32, 4), SEAL256: (0, 3)}))
    assert _guard(str(path)).returncode != 0


def test_build_runs_the_guard():
    """the library's link rule runs the guard over every kernel file's report first, so a build that loses the occupancy
    or the scratch ceiling fails; the reports a build left next to the sources (not part of a checkout) pass it"""
    rule = re.search(r"^\$\(OUT\):.*\n((?:\t.*\n)+)", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert rule, "no link rule in csrc/Makefile"
    steps = rule.group(1).splitlines()
    guard = [i for i, step in enumerate(steps) if "check_resources.py $(SRC_HIP:.hip=.res)" in step]
    link = [i for i, step in enumerate(steps) if "-shared" in step]
    assert guard and link and guard[0] < link[0], steps
    res = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".res"))
    if res:
        r = _guard(*res)
        assert r.returncode == 0, r.stderr
