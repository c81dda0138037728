"""train.py's TensorBoard summaries without TensorFlow or tensorboard: the event file written by hand, like ckpt_export.py's bundle.

An event file is a TFRecord file (tfrecords.py's framing: length, masked CRC-32C of the length, payload, masked CRC-32C) of Event
messages.  The first holds file_version "brain.Event:2"; every other one a step and a Summary of scalars and histograms:

    Event            wall_time = 1 (double)   step = 2 (int64)   file_version = 3 (string)   summary = 5 (Summary)
    Summary          value = 1 (repeated Value)
    Summary.Value    tag = 1 (string)   simple_value = 2 (float)   histo = 5 (HistogramProto)
    HistogramProto   min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 (double)   bucket_limit = 6, bucket = 7 (packed double)

A histogram is what ssd_train_histograms computed (include/ssd_hip.h, "the TRAIN step's histograms": counts over
train_calls.histogram_limits() and the ssd_histogram_stats), compressed the way TF's Histogram::EncodeToProto does: a run of empty
buckets collapses into its last bucket with count 0, every non-empty bucket is written with its limit.
"""
import os
import socket
import struct
import time

import numpy as np

from .ckpt_export import _field_bytes, _varint
from .ckpt_import import masked_crc32c
from .pb_import import _fields
from .tfrecords import read_records

FILE_VERSION = "brain.Event:2"


def _double(number, v):
    return _varint(number << 3 | 1) + struct.pack("<d", float(v))


def _packed_doubles(number, values):
    return _field_bytes(number, np.asarray(values, "<f8").tobytes())


def compress_buckets(limits, counts):
    """(bucket_limit, bucket) float64 arrays of one plane: TF's compression of the empty runs."""
    limits, counts = np.asarray(limits, np.float64), np.asarray(counts)
    if limits.ndim != 1 or counts.shape != limits.shape:
        raise ValueError("limits and counts must be 1-D arrays of one length")
    if len(counts) == 0:
        return limits, counts.astype(np.float64)
    nonzero = counts != 0
    # bucket i is written when it is not empty, or when it ends a run of empty ones (its successor is not empty, or it is the last)
    keep = nonzero | np.append(nonzero[1:], True)
    return limits[keep], counts[keep].astype(np.float64)


def histogram_proto(limits, counts, stats):
    """HistogramProto bytes of one plane: limits float64 [NB], counts integers [NB], stats a record or mapping with sum, sum_squares,
    min, max, num and bad (train_calls.STATS_DTYPE).  A plane with a non-finite element raises FloatingPointError, as TF's "Nan in
    summary histogram" does."""
    if int(stats["bad"]) > 0:
        raise FloatingPointError("Nan in summary histogram: %d non-finite element(s)" % int(stats["bad"]))
    lim, bkt = compress_buckets(limits, counts)
    return (_double(1, stats["min"]) + _double(2, stats["max"]) + _double(3, int(stats["num"])) + _double(4, stats["sum"]) +
            _double(5, stats["sum_squares"]) + _packed_doubles(6, lim) + _packed_doubles(7, bkt))


def _value(tag, scalar=None, histo=None):
    body = _field_bytes(1, tag.encode())
    if histo is not None:
        body += _field_bytes(5, bytes(histo))
    else:
        body += _varint(2 << 3 | 5) + struct.pack("<f", float(scalar))
    return _field_bytes(1, body)


class EventFileWriter:
    """logdir/events.out.tfevents.<10-digit seconds>.<hostname>, opened with the version record; add_summary appends one Event and
    flushes the file."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        base = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
        path, n = base, 0
        while True:                                                  # a second writer of the same second gets a suffix of its own
            try:
                self._f = open(path, "xb")
                break
            except FileExistsError:
                n += 1
                path = "%s.%d" % (base, n)
        self.path = path
        self._write(_double(1, now) + _field_bytes(3, FILE_VERSION.encode()))

    def _write(self, event):
        event = bytes(event)
        head = struct.pack("<Q", len(event))
        self._f.write(head + struct.pack("<I", masked_crc32c(head)) + event + struct.pack("<I", masked_crc32c(event)))
        self._f.flush()

    def add_summary(self, step, scalars=None, histograms=None, wall_time=None):
        """One Event at `step`: scalars {tag: number} as simple_value (float32), histograms {tag: histogram_proto bytes}."""
        summary = b"".join(_value(tag, scalar=v) for tag, v in (scalars or {}).items())
        summary += b"".join(_value(tag, histo=h) for tag, h in (histograms or {}).items())
        self._write(_double(1, time.time() if wall_time is None else wall_time) + _varint(2 << 3) + _varint(int(step)) +
                    _field_bytes(5, summary))

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _parse_histogram(buf):
    out = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for fn, wt, v in _fields(buf):
        if fn in names and wt == 1:
            out[names[fn]] = struct.unpack("<d", struct.pack("<Q", v))[0]
        elif fn in (6, 7):
            key = "bucket_limit" if fn == 6 else "bucket"
            if wt == 2:
                out[key] += np.frombuffer(bytes(v), "<f8").tolist()
            elif wt == 1:
                out[key].append(struct.unpack("<d", struct.pack("<Q", v))[0])
    return out


def read_events(path):
    """The summary events of one event file: a list of (wall_time, step, {tag: float | dict of the histogram's fields (min, max, num,
    sum, sum_squares, bucket_limit, bucket)}).  Both CRCs of every record are verified; the first record must be the version record."""
    events = []
    for i, rec in enumerate(read_records(path, verify=True)):
        wall, step, version, values = 0.0, 0, None, None
        for fn, wt, v in _fields(memoryview(rec)):
            if fn == 1 and wt == 1:
                wall = struct.unpack("<d", struct.pack("<Q", v))[0]
            elif fn == 2 and wt == 0:
                step = v - (1 << 64) if v >> 63 else v
            elif fn == 3 and wt == 2:
                version = bytes(v).decode()
            elif fn == 5 and wt == 2:
                values = {} if values is None else values
                for fn2, wt2, val in _fields(v):
                    if fn2 != 1 or wt2 != 2:
                        continue
                    tag, content = None, None
                    for fn3, wt3, x in _fields(val):
                        if fn3 == 1 and wt3 == 2:
                            tag = bytes(x).decode()
                        elif fn3 == 2 and wt3 == 5:
                            content = struct.unpack("<f", struct.pack("<I", x))[0]
                        elif fn3 == 5 and wt3 == 2:
                            content = _parse_histogram(x)
                    if tag is not None:
                        values[tag] = content
        if i == 0:
            if version != FILE_VERSION:
                raise ValueError("%s: the first record is not the %r version record" % (path, FILE_VERSION))
            continue
        if values is not None:
            events.append((wall, step, values))
    return events


def event_files(logdir):
    """The event files of a directory, in name (= time) order."""
    if not os.path.isdir(logdir):
        return []
    return [os.path.join(logdir, f) for f in sorted(os.listdir(logdir)) if f.startswith("events.out.tfevents.")]
