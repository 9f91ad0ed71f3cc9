"""bench.py as a program: the result line of a plain run and of --full, and --dump-outputs against the oracle.

Two short runs of a small batch (16403 packets: just past the 16384 up to which the burst kernels run, so the
headline's quad kernel runs; not a multiple of the 16 packets of a wave) with different step counts: the dumped
arrays must be the same in both (seeded inputs), float32, and equal to what the oracle computes from the same
inputs: the arena after seal + open is [AAD | plaintext | the seal's tag], with the seal's HP masks beside it and
every status 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import qpp
from conftest import ROOT

pytestmark = pytest.mark.gpu
N, PT, AAD = 16403, 1200, 21
SEED = 0x5eed0000 + 1  # bench.py: the key secret's generator and rank 0's shard seed


def run_bench(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--packets", str(N),
                        "--dump-outputs", str(out), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bench")
    return (run_bench(tmp, "plain", "--steps", "3", "--warmup", "1"),
            run_bench(tmp, "full", "--steps", "1", "--warmup", "1", "--full", "--cpu-seconds", "0.05"))


def test_result_line(runs):
    (plain, _), (full, _) = runs
    for line, steps, warmup in ((plain, 3, 1), (full, 1, 1)):
        assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
        assert line["steps"] == steps and line["warmup"] == warmup
        assert line["ms_per_step"] > 0
        # value = seal + open payload bytes of all timed steps over their time
        assert line["value"] == pytest.approx(2.0 * N * PT / (line["ms_per_step"] / 1e3) / (1 << 30), rel=1e-2)
    assert plain["cpu_baseline"] is None  # the CPU leg runs under --full only
    assert full["cpu_baseline"]["value"] > 0 and "verified=True" in full["cpu_baseline"]["sample"]


def test_dump_is_reproducible_and_matches_the_oracle(runs):
    (_, a), (_, b) = runs
    assert sorted(a) == sorted(b) == ["hp_masks", "packet_index", "packets", "status"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert a[name].shape == b[name].shape and (a[name] == b[name]).all(), name
    assert sum(x.nbytes for x in a.values()) <= 64e6
    idx = a["packet_index"].astype(np.int64)
    assert len(idx) == 8012 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < N  # 40 MB of float32 rows
    assert a["status"].shape == (N,) and (a["status"] == 0).all()

    with qpp.Context(0) as ctx:
        k = ctx.key(1, np.random.default_rng(SEED).integers(0, 256, qpp.HASH_LEN[1], dtype=np.uint8).tobytes())
        okeys = orc.make_keys([(1, *k.material())])
        k.free()
    descs, arena = qpp.make_batch(N, PT, [0], seed=SEED, aad_len=AAD)
    want = arena.copy()
    want_masks = orc.seal_batch(okeys, descs, want, qpp.HP_MASK_OUT)
    stride = arena.size // N
    want, arena = want.reshape(N, stride)[idx], arena.reshape(N, stride)[idx]
    assert (want[:, AAD + PT:AAD + PT + 16] != arena[:, AAD + PT:AAD + PT + 16]).any(axis=1).all()  # tags written
    want[:, :AAD + PT] = arena[:, :AAD + PT]  # the open puts the plaintext back and leaves the tag
    assert (a["packets"] == want).all()
    want_masks = np.frombuffer(want_masks, np.uint8).reshape(N, 5)[idx]
    assert (a["hp_masks"] == want_masks).all()
