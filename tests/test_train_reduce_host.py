"""The TRAIN step's gradient exchange without a GPU (include/ssd_hip.h): the bucket layout, every refusal of
ssd_train_grad_pack / ssd_train_grad_reduce (all come before any HIP call), TrainPipeline's shard= selection, and the digest that
keeps ranks with different tables from exchanging (two gloo CPU ranks)."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from helpers import train_reduce_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "helpers", "grad_exchange_worker.py")
COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097)


def _table(train_calls, counts, base=0x100000):
    rows = np.zeros(len(counts), train_calls.REDUCE_ROW_DTYPE)
    rows["count"] = counts
    rows["offset"] = ref.bucket_layout(counts)[0]
    rows["data"] = [base + 0x100000 * i for i in range(len(counts))]         # never dereferenced; 1 MiB apart: no overlap below 2^18 floats
    return rows


def test_bucket_layout_is_pinned(ssd):
    from ssd_amd import train_calls
    L = ssd.lib()
    # every count alone: the row starts at 0, the payload is the count rounded up to 4 and then to 4096
    for n, floats in zip(COUNTS, (16, 16 + 4096, 16 + 4096, 16 + 4096, 16 + 4096, 16 + 4096, 16 + 4096, 16 + 8192)):
        offsets, P, slice_floats = ref.bucket_layout([n])
        assert (offsets, slice_floats) == ([0], floats) and P == floats - 16
        got = train_calls.bucket_layout([n])
        assert got[0].tolist() == [0] and got[1] == floats
        rows = _table(train_calls, [n])
        assert L.ssd_train_bucket_floats(rows.ctypes.data_as(ctypes.c_void_p), 1) == floats
    # ... and as one table, written out by hand: 0, 4, 4, 4, 8, 4096, 4096, 4100 bucket floats
    want = [0, 0, 4, 8, 12, 20, 4116, 8212]
    assert ref.bucket_layout(COUNTS) == (want, 16384, 16400)
    got = train_calls.bucket_layout(COUNTS)
    assert got[0].dtype == np.int64 and got[0].tolist() == want and got[1] == 16400
    rows = _table(train_calls, COUNTS)
    assert L.ssd_train_bucket_floats(rows.ctypes.data_as(ctypes.c_void_p), len(COUNTS)) == 16400
    # the layout depends on the counts alone: other addresses, NULL rows and kinds leave it as it is
    rows["data"][2], rows["kind"][5] = 0, 1
    rows["data"][6] += 4
    assert L.ssd_train_bucket_floats(rows.ctypes.data_as(ctypes.c_void_p), len(COUNTS)) == 16400
    # a table the calls would refuse has no size
    rows["offset"][3] += 4
    assert L.ssd_train_bucket_floats(rows.ctypes.data_as(ctypes.c_void_p), len(COUNTS)) == 0
    assert L.ssd_train_bucket_floats(None, 1) == 0
    with pytest.raises(ValueError):
        train_calls.bucket_layout([3, -1])
    with pytest.raises(ValueError):
        train_calls.bucket_layout([])


def test_pack_and_reduce_refuse_bad_arguments_without_a_gpu(ssd):
    from ssd_amd import train_calls
    L = ssd.lib()
    rows = _table(train_calls, (5000, 10, 4096))
    floats = 16 + 3 * 4096
    assert ref.bucket_layout(rows["count"])[2] == floats
    p = ctypes.c_void_p

    def pack(r=rows, dev=p(0x20000), T=3, header=p(0x30000), slice_=p(0x40000), n=floats):
        return L.ssd_train_grad_pack(r.ctypes.data_as(p) if r is not None else None, dev, T, header, slice_, n, None)

    def reduce(r=rows, dev=p(0x20000), T=3, gathered=p(0x40000), G=2, n=floats, losses=p(0x50000), weights=p(0x50010)):
        return L.ssd_train_grad_reduce(r.ctypes.data_as(p) if r is not None else None, dev, T, gathered, G, n, losses, weights, None)
    cases = {pack: ({"r": None}, {"dev": None}, {"header": None}, {"slice_": None}, {"T": 0}, {"T": -1}, {"T": 65537},
                    {"dev": p(0x20004)}, {"header": p(0x30002)}, {"slice_": p(0x40008)}, {"slice_": p(0x40004)},
                    {"n": floats - 4096}, {"n": floats + 4096}, {"n": floats - 16}, {"n": 0}),
             reduce: ({"r": None}, {"dev": None}, {"gathered": None}, {"losses": None}, {"weights": None}, {"T": 0}, {"T": -1},
                      {"T": 65537}, {"dev": p(0x20004)}, {"gathered": p(0x40008)}, {"losses": p(0x50002)}, {"weights": p(0x50011)},
                      {"G": 0}, {"G": -1}, {"G": 17}, {"n": floats - 4096}, {"n": floats + 4096}, {"n": 0})}
    names = {pack: "ssd_train_grad_pack", reduce: "ssd_train_grad_reduce"}
    for call, kws in cases.items():
        for kw in kws:
            assert call(**kw) == -1, (names[call], kw)
            assert L.ssd_last_error().decode().startswith(names[call]), kw
        for field, value, word in (("count", -1, "count"), ("count", (1 << 40) + 1, "count"), ("data", 0x200002, "aligned"),
                                   ("data", 0x200001, "aligned"), ("kind", 2, "kind"), ("kind", -1, "kind"),
                                   ("offset", 5004, "offset must be 5000"), ("offset", 0, "offset must be 5000")):
            q = rows.copy()
            q[1][field] = value
            assert call(r=q) == -1, (names[call], field)
            msg = L.ssd_last_error().decode()
            assert msg.startswith(names[call]) and "row 1" in msg and word in msg, (field, msg)
        # data ranges that overlap: row 2 starts inside row 0, by one element; touching ranges and NULL rows are fine up to here
        q = rows.copy()
        q[2]["data"] = q[0]["data"] + 4 * 4999
        assert call(r=q) == -1 and "overlap" in L.ssd_last_error().decode()
        q[1]["data"] = q[0]["data"]                      # the same start
        q[2]["data"] = rows[2]["data"]
        assert call(r=q) == -1 and "overlap" in L.ssd_last_error().decode()
    # the G the reduce takes: 1 .. 16 pass the check of G and reach the next one (here: a wrong slice size)
    for G in (1, 16):
        assert reduce(G=G, n=floats + 4) == -1 and "slice_floats must be %d" % floats in L.ssd_last_error().decode()


def test_train_pipeline_shard_selects_every_world_th_file_and_refuses_an_empty_share(ssd, tmp_path):
    d = tmp_path / "train"
    d.mkdir()
    for k in (3, 0, 4, 1, 2):
        (d / ("train-%02d.tfrecords" % k)).write_bytes(b"")
    (d / "notes.txt").write_bytes(b"")
    cfg = {"batch_size": 2, "image_height": 128, "image_width": 128}
    names = lambda p: [os.path.basename(s) for s in p.shards]
    every = ["train-%02d.tfrecords" % k for k in range(5)]
    assert names(ssd.TrainPipeline(str(d), cfg, seed=0)) == every == names(ssd.TrainPipeline(str(d), cfg, seed=0, shard=None))
    assert names(ssd.TrainPipeline(str(d), cfg, seed=0, shard=(0, 1))) == every
    for world in (2, 3, 5):
        got = [names(ssd.TrainPipeline(str(d), cfg, seed=0, shard=(r, world))) for r in range(world)]
        assert got == [every[r::world] for r in range(world)]
        assert sorted(n for g in got for n in g) == every
    with pytest.raises(ValueError, match="rank 5 of 6 gets no shard"):
        ssd.TrainPipeline(str(d), cfg, seed=0, shard=(5, 6))
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank, world"):
            ssd.TrainPipeline(str(d), cfg, seed=0, shard=bad)
    one = d / "train-00.tfrecords"                       # a single file is one shard: rank 1 of 2 gets none
    assert names(ssd.TrainPipeline(str(one), cfg, seed=0, shard=(0, 2))) == ["train-00.tfrecords"]
    with pytest.raises(ValueError, match="gets no shard"):
        ssd.TrainPipeline(str(one), cfg, seed=0, shard=(1, 2))


def test_ranks_with_different_tables_both_raise(tmp_path):
    """Two gloo CPU ranks (children under a time limit): equal tables pass, and for each of three differences -- a count, which
    gradient is present, the number of rows -- BOTH ranks raise ValueError."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, "digest", str(tmp_path)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=120)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)
    for rank in range(2):
        assert (tmp_path / ("digest_rank%d.ok" % rank)).read_text() == "raised 3\n"
