"""train.py's summaries without a GPU: ssd_histogram_limits against the restated loop, the numpy restatement's buckets at the edges,
histogram_proto's compression, the event file (framing, read_events, and a second decoder built on google.protobuf from a hand-made
descriptor), the summary schedule, and every refusal of ssd_train_histograms and its planner (all come before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import histogram_ref as ref

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------- the limits
def test_the_library_limits_are_the_restated_loop_bit_for_bit(ssd):
    L = ssd.lib()
    NB = L.ssd_histogram_limits(None, 0)
    assert NB == ref.NB == len(ref.LIMITS) and NB % 2 == 1
    buf = np.full(NB + 2, 7.0, f64)
    assert L.ssd_histogram_limits(buf[1:].ctypes.data, NB - 1) == NB and (buf == 7.0).all()      # a short capacity writes nothing
    assert L.ssd_histogram_limits(buf[1:].ctypes.data, NB) == NB
    assert buf[0] == 7.0 and buf[-1] == 7.0
    got = buf[1:-1]
    assert np.array_equal(got.view(np.int64), ref.LIMITS.view(np.int64))
    assert (np.diff(got) > 0).all()
    M = NB // 2
    assert got[M] == 0.0 and np.array_equal(got[:M], -got[:M:-1]) and got[-1] == np.finfo(f64).max
    assert got[M + 1] == 1e-12 and got[-2] < 1e20 <= got[-2] * 1.1
    table = ssd.histogram_limits()
    assert table.dtype == f64 and not table.flags.writeable and np.array_equal(table.view(np.int64), ref.LIMITS.view(np.int64))
    assert ssd.train_calls.histogram_limits() is table


def test_the_restatement_buckets_at_the_edges():
    M = ref.NB // 2
    c, st = ref.plane(np.array([0.0, -0.0, 1e-45, -1e-45, np.finfo(f32).max, -np.finfo(f32).max, np.nan, np.inf, -np.inf], f32), 1)
    assert c[M + 1] == 3 and c[M] == 1                               # both zeros and the positive denormal; the negative denormal
    assert c.sum() == 6 and st["num"] == 6 and st["bad"] == 3
    assert st["min"] == -np.finfo(f32).max and st["max"] == np.finfo(f32).max
    top = np.nonzero(c)[0]
    assert ref.LIMITS[top[-1]] > np.finfo(f32).max >= ref.LIMITS[top[-1] - 1]
    assert ref.LIMITS[top[0]] > -np.finfo(f32).max >= ref.LIMITS[top[0] - 1]
    # an element equal to a limit belongs to the bucket ABOVE it (the first limit strictly greater)
    # (0.0 is the only limit that is a float32: both zeros went to bucket M + 1 above)
    with np.errstate(over="ignore"):
        assert np.nonzero(ref.LIMITS == ref.LIMITS.astype(f32).astype(f64))[0].tolist() == [M]
    # min and max order -0.0 below +0.0, whatever the element order
    for x in ([0.0, -0.0], [-0.0, 0.0]):
        st = ref.plane(np.array(x, f32), 0)[1]
        assert np.signbit(st["min"]) and not np.signbit(st["max"])
    c, st = ref.plane(np.zeros(0, f32), 2)
    assert c.sum() == 0 and st["min"] == np.inf and st["max"] == -np.inf and st["num"] == 0 and st["sum_squares"] == 0.0


def test_the_gradient_plane_is_one_multiply_and_one_add():
    w, g = np.array([3.0, 1e30, -2.0], f32), np.array([1.0, 1e38, np.nan], f32)
    got = ref.gradient_plane(w, g, 1, 0.1)
    assert got[0] == f32(1.0) + f32(f32(0.1) * f32(3.0)) and np.isnan(got[2])
    assert np.array_equal(ref.gradient_plane(w, g, 0, 0.1), g, equal_nan=True)
    counts, stats = ref.table_histograms([(w, g, 0, 1), (w, None, 3, 1)], 0.1)
    assert stats[0, 1]["bad"] == 1 and stats[0, 1]["num"] == 2 and stats[1, 1]["num"] == 0 and counts[1, 1].sum() == 0
    assert stats[1, 1]["min"] == np.inf and stats[1, 1]["max"] == -np.inf


# ----------------------------------------------------------------------------- histogram_proto
def _stats(num=0, bad=0, lo=np.inf, hi=-np.inf, s=0.0, q=0.0):
    st = np.zeros((), ref.STATS_DTYPE)
    st["num"], st["bad"], st["min"], st["max"], st["sum"], st["sum_squares"] = num, bad, lo, hi, s, q
    return st


def _decode_histogram(buf):
    from ssd_amd import summaries
    return summaries._parse_histogram(memoryview(buf))


def test_histogram_proto_compresses_runs_of_empty_buckets(ssd):
    from ssd_amd import summaries
    NB, limits = ref.NB, ref.LIMITS
    # all empty: one bucket, the last limit, count 0
    h = _decode_histogram(summaries.histogram_proto(limits, np.zeros(NB, np.int64), _stats()))
    assert h["bucket_limit"] == [float(limits[-1])] and h["bucket"] == [0.0]
    assert h["num"] == 0 and h["min"] == np.inf and h["max"] == -np.inf
    # one non-empty bucket at each end: the run between them collapses into its last bucket
    c = np.zeros(NB, np.int64)
    c[0], c[-1] = 3, 5
    h = _decode_histogram(summaries.histogram_proto(limits, c, _stats(8, 0, -1.0, 1.0, 2.0, 8.0)))
    assert h["bucket_limit"] == [float(limits[0]), float(limits[-2]), float(limits[-1])] and h["bucket"] == [3.0, 0.0, 5.0]
    assert (h["num"], h["min"], h["max"], h["sum"], h["sum_squares"]) == (8.0, -1.0, 1.0, 2.0, 8.0)
    # alternating runs: empty x2, full x2, empty x3, full x1, empty to the end
    c = np.zeros(NB, np.int64)
    c[[2, 3, 7]] = [1, 2, 4]
    h = _decode_histogram(summaries.histogram_proto(limits, c, _stats(7)))
    assert h["bucket_limit"] == [float(limits[i]) for i in (1, 2, 3, 6, 7, NB - 1)] and h["bucket"] == [0.0, 1.0, 2.0, 0.0, 4.0, 0.0]
    for case in (np.zeros(NB, np.int64), c):
        lim, bkt = summaries.compress_buckets(limits, case)
        want = ref.compressed(case)
        assert lim.tolist() == want[0] and bkt.tolist() == want[1]
    with pytest.raises(FloatingPointError, match="Nan in summary histogram"):
        summaries.histogram_proto(limits, c, _stats(7, bad=1))


# ----------------------------------------------------------------------------- the event file
def _events(ssd, directory):
    from ssd_amd import summaries
    rng = np.random.default_rng(0)
    x = (rng.normal(0, 0.05, 5000)).astype(f32)
    counts, st = ref.plane(x, 0)
    written = []
    with summaries.EventFileWriter(str(directory)) as w:
        path = w.path
        for step in (1, 2, 700):
            scalars = {"loss": float(f32(1.5 / step)), "learning_rate/learning_rate": float(f32(1e-3)), "global_step/sec": float(f32(step))}
            w.add_summary(step, scalars, {"v/weights_hist": summaries.histogram_proto(ref.LIMITS, counts, st)}, wall_time=1e9 + step)
            written.append((1e9 + step, step, scalars))
        w.add_summary(0, {"only": 2.0}, None, wall_time=5.0)
        written.append((5.0, 0, {"only": 2.0}))
    return path, written, (counts, st, x)


def test_the_event_file_frames_and_reads_back(ssd, tmp_path):
    from ssd_amd import summaries, tfrecords
    path, written, (counts, st, x) = _events(ssd, tmp_path / "logs")
    assert re.match(r"^events\.out\.tfevents\.\d{10}\.%s$" % re.escape(__import__("socket").gethostname()), os.path.basename(path))
    assert summaries.event_files(str(tmp_path / "logs")) == [path]
    records = list(tfrecords.read_records(path, verify=True))
    assert len(records) == 1 + len(written) and b"brain.Event:2" in records[0]
    events = summaries.read_events(path)
    assert [(w, s) for w, s, _v in events] == [(w, s) for w, s, _v in written]
    lim, bkt = ref.compressed(counts)
    for (_w, _s, got), (_w2, _s2, scalars) in zip(events, written):
        for tag, v in scalars.items():
            assert got[tag] == v, tag
        if "v/weights_hist" in got:
            h = got["v/weights_hist"]
            assert h["bucket_limit"] == lim and h["bucket"] == bkt and sum(bkt) == 5000
            assert h["num"] == 5000 and h["min"] == float(x.min()) and h["max"] == float(x.max())
            assert h["sum"] == float(st["sum"]) and h["sum_squares"] == float(st["sum_squares"])
    assert "v/weights_hist" not in events[-1][2]
    # a second writer of the same directory never appends to the first one's file
    with summaries.EventFileWriter(str(tmp_path / "logs")) as w2:
        assert w2.path != path
    # a damaged byte is found
    raw = bytearray(open(path, "rb").read())
    raw[40] ^= 1
    bad = tmp_path / "damaged"
    bad.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="CRC|corrupt"):
        summaries.read_events(str(bad))


def _event_class():
    """Event, Summary and HistogramProto from a hand-made FileDescriptorProto with the documented field numbers."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="ssd_summary_test.proto", package="ssdtest", syntax="proto3")

    def message(name, fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, type_name in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if type_name:
                f.type_name = ".ssdtest." + type_name
        return m
    ONE, MANY = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    message("HistogramProto", [("min", 1, F.TYPE_DOUBLE, ONE, None), ("max", 2, F.TYPE_DOUBLE, ONE, None), ("num", 3, F.TYPE_DOUBLE, ONE, None),
                               ("sum", 4, F.TYPE_DOUBLE, ONE, None), ("sum_squares", 5, F.TYPE_DOUBLE, ONE, None),
                               ("bucket_limit", 6, F.TYPE_DOUBLE, MANY, None), ("bucket", 7, F.TYPE_DOUBLE, MANY, None)])
    message("Value", [("tag", 1, F.TYPE_STRING, ONE, None), ("simple_value", 2, F.TYPE_FLOAT, ONE, None),
                      ("histo", 5, F.TYPE_MESSAGE, ONE, "HistogramProto")])
    message("Summary", [("value", 1, F.TYPE_MESSAGE, MANY, "Value")])
    message("Event", [("wall_time", 1, F.TYPE_DOUBLE, ONE, None), ("step", 2, F.TYPE_INT64, ONE, None),
                      ("file_version", 3, F.TYPE_STRING, ONE, None), ("summary", 5, F.TYPE_MESSAGE, ONE, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("ssdtest.Event"))


def test_a_protobuf_decoder_reads_the_same_values(ssd, tmp_path):
    pytest.importorskip("google.protobuf")
    from ssd_amd import summaries, tfrecords
    Event = _event_class()
    path, written, _ = _events(ssd, tmp_path / "logs")
    records = list(tfrecords.read_records(path, verify=True))
    first = Event.FromString(records[0])
    assert first.file_version == "brain.Event:2" and first.wall_time > 1e9 and not first.HasField("summary")
    mine = summaries.read_events(path)
    assert len(mine) == len(records) - 1 == len(written)
    for rec, (wall, step, values) in zip(records[1:], mine):
        e = Event.FromString(rec)
        assert e.wall_time == wall and e.step == step and e.file_version == ""
        assert [v.tag for v in e.summary.value] == list(values)
        for v in e.summary.value:
            if v.HasField("histo"):
                h, want = v.histo, values[v.tag]
                assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (want["min"], want["max"], want["num"], want["sum"], want["sum_squares"])
                assert list(h.bucket_limit) == want["bucket_limit"] and list(h.bucket) == want["bucket"]
            else:
                assert v.simple_value == values[v.tag]


# ----------------------------------------------------------------------------- the schedule
def test_summary_due(ssd):
    from ssd_amd.trainer import summary_due
    assert summary_due(1, None, 600) and summary_due(12345, None, 600)            # the first step of a run, fresh or resumed
    assert not summary_due(2, 1, 600) and not summary_due(600, 1, 600) and summary_due(601, 1, 600)
    assert not summary_due(12346, 12345, 600) and summary_due(12945, 12345, 600)
    assert all(summary_due(s, s - 1, 1) for s in range(2, 6))                     # every = 1: every step
    for start, every, want in ((1, 2, [1, 3, 5, 7]), (41, 3, [41, 44, 47]), (1, 1, [1, 2, 3, 4, 5, 6, 7])):
        last, got = None, []
        for s in range(start, start + 7):
            if summary_due(s, last, every):
                got.append(s)
                last = s
        assert got == want, (start, every)
    assert not summary_due(1, None, 0) and not summary_due(10 ** 6, 1, 0)         # 0: never
    with pytest.raises(ValueError):
        summary_due(1, None, -1)


def test_the_train_command_takes_the_option(ssd):
    import inspect
    from ssd_amd import trainer
    assert trainer.SAVE_SUMMARY_STEPS == 600
    for fn in (trainer.Trainer.train, trainer.Trainer.train_and_evaluate):
        assert inspect.signature(fn).parameters["save_summary_steps"].default == 0
    r = {"loss": 1.0, "regularization_loss": 2.0, "localization_loss": 3.0, "classification_loss": 4.0, "learning_rate": 5.0, "step": 9}
    assert trainer.summary_scalars(r) == {"loss": 1.0, "regularization_loss": 2.0, "localization_loss": 3.0, "classification_loss": 4.0,
                                          "learning_rate/learning_rate": 5.0}
    assert trainer.summary_scalars(r, 2.5)["global_step/sec"] == 2.5
    rows = np.array([[0.5, 0.25, 7, 4, 2, 1, 0, 0], [0.5, 0.25, 4, 1, 1, 1, 1, 0]], f32)      # per image: loc, cls, matches, levels 3 .. 7
    got = trainer.summary_scalars(r, None, rows)
    scope = "losses/loss_summaries/"
    assert [got[scope + "mean_matches_per_image_on_level_%d" % l] for l in range(3, 8)] == [2.5, 1.5, 1.0, 0.5, 0.0]
    assert got[scope + "total_mean_matches_per_image"] == 5.5 and len(got) == 5 + 6


# ----------------------------------------------------------------------------- the refusals
def _rows(train_step):
    rows = np.zeros(3, train_step.TENSOR_DTYPE)
    for c in ("w", "grad", "m", "v", "ema"):
        rows[c] = 0x10000                       # never dereferenced: every refusal comes before any HIP call
    rows["count"] = (5000, 10, 4096)
    rows["decay"] = (1, 0, 0)
    rows["first_block"] = (0, 2, 3)
    return rows


def test_the_histograms_refuse_what_the_update_refuses_and_their_own_arguments(ssd):
    from ssd_amd import train_step
    L = ssd.lib()
    rows = _rows(train_step)
    fake, out = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    NEED = 4 * 64                               # 2 + 1 + 1 blocks

    def plan(r=rows, T=3):
        return L.ssd_train_histograms_workspace_bytes(r.ctypes.data_as(ctypes.c_void_p) if r is not None else None, T)

    def call(r=rows, dev=fake, T=3, wd=1e-4, limits=out, counts=out, stats=out, ws=fake, nbytes=NEED):
        return L.ssd_train_histograms(r.ctypes.data_as(ctypes.c_void_p) if r is not None else None, dev, T, wd, limits, counts, stats, ws,
                                      nbytes, None)
    assert plan() == NEED == 64 * train_step.block_starts(rows["w"], rows["count"])[1]
    for kw in ({"r": None}, {"dev": None}, {"T": 0}, {"T": -1}, {"T": 65537}, {"dev": ctypes.c_void_p(0x20004)}):
        assert call(**kw) == -1, kw
        assert L.ssd_last_error().decode().startswith("ssd_train_histograms:"), kw
        if "dev" not in kw:
            assert plan(**kw) == 0, kw
    for field, value, word in (("count", -1, "count"), ("count", (1 << 40) + 1, "count"), ("w", 0, "NULL"), ("m", 0, "NULL"),
                               ("v", 0, "NULL"), ("ema", 0, "NULL"), ("w", 0x10002, "aligned"), ("m", 0x10001, "aligned"),
                               ("v", 0x10003, "aligned"), ("ema", 0x10002, "aligned"), ("grad", 0x10002, "aligned"),
                               ("decay", 2, "decay"), ("first_block", 1, "first_block")):
        q = rows.copy()
        q[1][field] = value
        assert call(r=q) == -1, field
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_train_histograms:") and "tensor 1" in msg and word in msg, (field, msg)
        assert plan(r=q) == 0, field
    odd = ctypes.c_void_p(0x30004)
    for kw, word in (({"wd": float("nan")}, "weight_decay"), ({"wd": float("inf")}, "weight_decay"),
                     ({"limits": None}, "NULL limits_dev"), ({"counts": None}, "NULL limits_dev"), ({"stats": None}, "NULL limits_dev"),
                     ({"limits": odd}, "8-byte aligned"), ({"counts": odd}, "8-byte aligned"), ({"stats": odd}, "8-byte aligned"),
                     ({"ws": None}, "NULL workspace"), ({"ws": ctypes.c_void_p(0x20008)}, "16-byte aligned"),
                     ({"nbytes": NEED - 1}, "too small"), ({"nbytes": 0}, "too small")):
        assert call(**kw) == -1, kw
        msg = L.ssd_last_error().decode()
        assert msg.startswith("ssd_train_histograms:") and word in msg, (kw, msg)
    q = rows.copy()
    q["grad"] = 0
    assert plan(r=q) == NEED                    # a NULL grad is no refusal
    q["count"], q["first_block"] = 0, 0
    assert plan(r=q) == 0                       # a table of empty tensors needs no workspace bytes


def test_the_call_layer_checks_its_tensors_on_the_cpu(ssd):
    import torch
    from ssd_amd import train_calls, train_step
    rows = torch.from_numpy(_rows(train_step).view(np.uint8).copy())
    NB = ref.NB
    assert train_calls.train_histograms_workspace_bytes(rows) == 4 * 64
    assert train_calls.STATS_DTYPE == ref.STATS_DTYPE and train_calls.STATS_BYTES == 40
    good = dict(rows_dev=torch.zeros(3 * 56, dtype=torch.uint8), limits_dev=torch.zeros(NB, dtype=torch.float64),
                counts=torch.zeros((3, 2, NB), dtype=torch.int64), stats=torch.zeros((3, 2, 40), dtype=torch.uint8))
    for name, wrong in (("rows_dev", torch.zeros(3 * 56 - 1, dtype=torch.uint8)), ("limits_dev", torch.zeros(NB - 1, dtype=torch.float64)),
                        ("limits_dev", torch.zeros(NB, dtype=torch.float32)), ("counts", torch.zeros((3, 2, NB), dtype=torch.int32)),
                        ("counts", torch.zeros((3, 1, NB), dtype=torch.int64)), ("stats", torch.zeros((3, 2, 48), dtype=torch.uint8))):
        with pytest.raises(ValueError, match=name):
            train_calls.train_histograms(rows, **dict(good, **{name: wrong}), weight_decay=1e-4)
    with pytest.raises(TypeError, match="GPU"):                      # last of the checks: there is no CPU path
        train_calls.train_histograms(rows, weight_decay=1e-4, **good)
    unset = -2 ** 31
    assert ssd.get_option("hist_scheme") == unset
    ssd.set_option("hist_scheme", 0)
    assert ssd.get_option("hist_scheme") == 0
    ssd.set_option("hist_scheme", unset)
