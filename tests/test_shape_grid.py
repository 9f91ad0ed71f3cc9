"""The shape grid (tests/_shapes.py) on the CPU: the two checkers -- the restatement (oracle/qpp_oracle.c) and OpenSSL
(oracle/fastcheck.c) -- agree on every packet of it, and the grid reaches the kernel edges it was made for.  The GPU
tests of the same grid (tests/test_gpu_shapes.py) compare the kernels with OpenSSL alone, so this is what ties their
expectations to the restatement of the reference."""
import numpy as np
import pytest

import _oracle as orc
import _shapes
import qpp

HP = qpp.HP_MASK_OUT | qpp.HP_APPLY


def _keys(suites, seed):
    rng = np.random.default_rng(seed)
    return orc.make_keys([(s, *orc.derive(s, rng.integers(0, 256, qpp.HASH_LEN[s], dtype=np.uint8).tobytes()))
                          for s in suites])


def _agree(keys, nkeys, cases, seed):
    """seal with header protection (arena, masks), seal without and the restatement's open of that, on `cases`"""
    descs, arena = _shapes.build_batch([c for c in cases if _shapes.hp_ok(c)], range(nkeys), seed)
    a, b = arena.copy(), arena.copy()
    m_a = orc.seal_batch(keys, descs, a, HP)
    m_b = orc.fast_seal_batch(keys, descs, b, HP)
    assert (a == b).all(), f"sealed arena differs, first at byte {int(np.flatnonzero(a != b)[0])}"
    assert m_a == m_b.tobytes()
    descs, arena = _shapes.build_batch(cases, range(nkeys), seed + 1, shuffle=True)
    assert len(descs) == len(cases)
    a, b = arena.copy(), arena.copy()
    orc.seal_batch(keys, descs, a, 0)
    orc.fast_seal_batch(keys, descs, b, 0)
    assert (a == b).all(), f"sealed arena differs, first at byte {int(np.flatnonzero(a != b)[0])}"
    assert orc.open_batch(keys, descs, b) == [qpp.OK] * len(descs)
    for d in descs:  # the plaintext is back; header and tag stay as sealed
        o, al, pl = int(d["off"]), int(d["aad_len"]), int(d["pt_len"])
        assert (b[o + al:o + al + pl] == arena[o + al:o + al + pl]).all()
        assert (b[o + al + pl:o + al + pl + 16] == a[o + al + pl:o + al + pl + 16]).all()
    return len(descs)


@pytest.mark.parametrize("suite", [1, 2, 3], ids=["aes128", "aes256", "chacha"])
def test_references_agree_on_the_grid(suite):
    cases = _shapes.grid_cases()
    assert _agree(_keys([suite, suite], 500 + suite), 2, cases, 600 + suite) == len(cases)


def test_references_agree_on_the_64k_rows():
    """once, over keys of all three suites (not per suite: the restatement takes a second per few MiB)"""
    cases = _shapes.big_rows()
    assert _agree(_keys([1, 2, 3], 504), 3, cases, 604) == len(cases)


def test_grid_reaches_what_it_is_for():
    cases = _shapes.grid_cases()
    for hp in (False, True):  # (every AES path runs both lists)
        sel = _shapes.grid_cases(hp=hp)
        assert sum(1 for c in sel if c[0] > 64) >= 50
        assert sum(1 for c in sel if _shapes.blocks(c[0], c[1])[0] >= 64) >= 10
    ms = {_shapes.blocks(c[0], c[1])[1] for c in _shapes.block_rows()}
    assert ms == set(_shapes.BLOCK_M)
    for a in _shapes.BLOCK_A:
        got = {_shapes.blocks(c[0], c[1])[1] for c in _shapes.block_rows() if _shapes.blocks(c[0], c[1])[0] == a}
        assert got == {m for m in _shapes.BLOCK_M if m - a - 1 >= 0}, a
    assert any(_shapes.blocks(c[0], c[1])[1] % 64 == 0 and _shapes.blocks(c[0], c[1])[0] > 4
               for c in _shapes.grid_cases(hp=True))
    # every grid value is there, with both PN lengths, and a header always holds its PN bytes
    for pn in _shapes.PN_LENS:
        assert {c[0] for c in cases if c[2] == pn} >= {pn if a is None else a for a in _shapes.AAD_LENS
                                                        if a != _shapes.BIG}
        assert {c[1] for c in cases if c[2] == pn} >= {p for p in _shapes.PT_LENS if p != _shapes.BIG}
    big = _shapes.big_rows()
    assert any(c[0] == _shapes.BIG for c in big) and any(c[1] == _shapes.BIG for c in big)
    assert all(1 <= c[2] <= 4 and c[0] >= c[2] for c in cases + big)
    assert all(_shapes.hp_ok(c) for c in _shapes.grid_cases(hp=True) + big)
    # the early-HP condition pt_len + pn_len >= 20 from both sides, for both PN lengths
    for pn in _shapes.PN_LENS:
        assert any(c[2] == pn and c[1] + pn < 20 for c in cases) and any(c[2] == pn and c[1] + pn == 20 for c in cases)
    # no case is dropped when the descriptors are built, in either order, and none overlaps its neighbour
    for shuffle in (False, True):
        descs, arena = _shapes.build_batch(cases, [7, 9], seed=1, shuffle=shuffle)
        assert len(descs) == len(cases)
        got = sorted(zip(descs["aad_len"].tolist(), descs["pt_len"].tolist(), descs["pn_len"].tolist()))
        assert got == sorted(cases)
        end = descs["off"].astype(np.int64) + descs["aad_len"] + descs["pt_len"] + 16
        assert (end[:-1] <= descs["off"][1:]).all() and int(end[-1]) + 64 == arena.size
        assert set(descs["key_idx"].tolist()) == {7, 9}
        assert (descs["pn"] >= 2**32).sum() == (len(cases) + 1) // 2
