"""Baseline JPEG bytes -> uint8 RGB frames in device memory, laid out as Engine.forward_mixed takes them (include/ssd_hip.h, block
"the JPEG decoder"): the marker structure and the Huffman decoding on the host (ssd_jpeg_info_read, ssd_jpeg_entropy: plain C,
called through ctypes, which releases the interpreter lock -- a caller's thread pool runs them in parallel), everything behind the
quantised coefficients in two launches on the GPU (ssd_jpeg_decode).  The frames are bit for bit what
PIL.Image.open(...).convert("RGB") gives; a file the decoder does not take (progressive, CMYK, other samplings, a damaged stream,
..) is REFUSED by index and stays with the caller's own reader -- nothing is decoded some other way behind the caller's back.

    dec = JpegDecoder(0)
    (flat, hw, offsets), refused = dec.decode_many(list_of_bytes)
    engine.forward_mixed((flat, hw_of_one_network_shape, offsets_of_them), records)

The way back is JpegEncoder (include/ssd_hip.h, block "the JPEG encoder"): uint8 RGB frames on the device -> the files PIL's
Image.save(format="jpeg") writes, byte for byte -- colour conversion, downsampling, forward DCT and quantisation in two launches
(ssd_jpeg_encode), the Huffman coding and the markers on the host (ssd_jpeg_emit, through ctypes as above).

    enc = JpegEncoder(0)
    blobs = enc.encode_many(frames, quality=75, sampling="420")        # frames: [H, W, 3] uint8 tensors, or decode_many's tuple
"""
import ctypes

import numpy as np

from ._lib import (SSD_ERR_INVALID, SSD_ERR_UNSUPPORTED, SSD_JPEG_SAMPLING_420, SSD_JPEG_SAMPLING_444, SsdJpegEncodeImage, SsdJpegImage,
                   SsdError, SsdJpegInfo, check, lib)
from .ssd import _ptr, _stream, _torch


def _up16(n):
    return (n + 15) & ~15


class _Batch:
    """A batch between begin() and finish(): its pinned slot, the first plan and the entropy jobs."""
    __slots__ = ("blobs", "slot", "taken", "infos", "plan", "jobs", "refused", "done")


class JpegDecoder:
    """One GPU's decoder.  Two pinned coefficient buffers in rotation: begin() entropy-decodes a batch into the free one while the
    batch before is still being uploaded and computed; finish() uploads it and enqueues the two launches on the current stream.
    At most two batches may be between begin() and finish().  Not thread-safe itself (the entropy jobs are)."""

    def __init__(self, device=0):
        torch = _torch()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self._slots = [{"pin": None, "ev": None, "open": False} for _ in range(2)]
        self._turn = 0

    @staticmethod
    def read_info(blob):
        """(status, SsdJpegInfo): status 0, SSD_ERR_UNSUPPORTED or SSD_ERR_INVALID."""
        info = SsdJpegInfo()
        return lib().ssd_jpeg_info_read(blob, len(blob), ctypes.byref(info)), info

    def begin(self, blobs, pool=None):
        """Parses every stream, lays the accepted ones out in a pinned buffer and entropy-decodes them into it: on `pool`
        (a concurrent.futures executor; returns at once, finish() waits) or, without one, here."""
        torch = _torch()
        slot = self._slots[self._turn]
        if slot["open"]:
            raise RuntimeError("JpegDecoder: two batches are already between begin() and finish()")
        self._turn ^= 1
        b = _Batch()
        b.blobs = [x if isinstance(x, bytes) else bytes(x) for x in blobs]
        b.slot, b.taken, b.infos, b.refused, b.done = slot, [], [], {}, False
        for i, blob in enumerate(b.blobs):
            rc, info = self.read_info(blob)
            if rc == 0:
                b.taken.append(i)
                b.infos.append(info)
            elif rc in (SSD_ERR_UNSUPPORTED, SSD_ERR_INVALID):
                b.refused[i] = rc
            else:
                check(rc)
        n = len(b.taken)
        infos_c = (SsdJpegInfo * max(n, 1))(*b.infos)
        plan = (SsdJpegImage * max(n, 1))()
        totals = (ctypes.c_int64 * 4)()
        check(lib().ssd_jpeg_plan(infos_c, n, plan, totals))
        b.plan = plan
        quant_at = _up16(2 * totals[0])
        table_at = _up16(quant_at + 2 * totals[1])
        need = table_at + ctypes.sizeof(SsdJpegImage) * max(n, 1)
        if slot["ev"] is not None:
            slot["ev"].synchronize()                    # the upload that last read this buffer
        if slot["pin"] is None or slot["pin"].numel() < need:
            cap = 1 << 20
            while cap < need:
                cap <<= 1
            slot["pin"] = torch.empty((cap,), dtype=torch.uint8).pin_memory()
        slot["open"] = True
        base = slot["pin"].data_ptr()
        slot["quant_at"], slot["table_at"], slot["need"] = quant_at, table_at, need
        fn = lib().ssd_jpeg_entropy

        def job(k):
            return fn(b.blobs[b.taken[k]], len(b.blobs[b.taken[k]]), ctypes.byref(infos_c[k]),
                      base + 2 * plan[k].coef_offset, base + quant_at + 2 * plan[k].quant_offset)
        b.jobs = [pool.submit(job, k) for k in range(n)] if pool is not None else [job(k) for k in range(n)]
        return b

    def finish(self, b):
        """-> ((flat uint8 CUDA tensor, [(H, W)...], byte offsets), refused): the frames of the accepted streams in input order --
        Engine.forward_mixed's tuple form -- and the refused positions as {index: status}.  Asynchronous on the current stream."""
        torch = _torch()
        if b.done:
            raise RuntimeError("JpegDecoder: finish() twice")
        b.done = True
        slot = b.slot
        try:
            rcs = [j if isinstance(j, int) else j.result() for j in b.jobs]
            keep = []
            for k, rc in enumerate(rcs):
                if rc == 0:
                    keep.append(k)
                elif rc in (SSD_ERR_UNSUPPORTED, SSD_ERR_INVALID):
                    b.refused[b.taken[k]] = rc
                else:
                    check(rc)
            n = len(keep)
            refused = dict(sorted(b.refused.items()))
            with torch.cuda.device(self.device):
                if n == 0:
                    return (torch.empty((0,), dtype=torch.uint8, device=self.device), [], []), refused
                # the survivors' table: the layout again, their coefficients where the first plan put them
                infos_c = (SsdJpegInfo * n)(*[b.infos[k] for k in keep])
                table = (SsdJpegImage * n)()
                totals = (ctypes.c_int64 * 4)()
                check(lib().ssd_jpeg_plan(infos_c, n, table, totals))
                for j, k in enumerate(keep):
                    table[j].coef_offset, table[j].quant_offset = b.plan[k].coef_offset, b.plan[k].quant_offset
                ctypes.memmove(slot["pin"].data_ptr() + slot["table_at"], table, ctypes.sizeof(table))
                used = slot["table_at"] + ctypes.sizeof(table)
                dev = torch.empty((used,), dtype=torch.uint8, device=self.device)
                dev.copy_(slot["pin"][:used], non_blocking=True)
                if slot["ev"] is None:
                    slot["ev"] = torch.cuda.Event()
                slot["ev"].record()
                ws = torch.empty((max(int(lib().ssd_jpeg_workspace_bytes(table, n)), 16),), dtype=torch.uint8, device=self.device)
                flat = torch.empty((max(int(totals[3]), 16),), dtype=torch.uint8, device=self.device)
                at = dev.data_ptr()
                check(lib().ssd_jpeg_decode(table, at + slot["table_at"], n, at, at + slot["quant_at"], _ptr(ws), _ptr(flat),
                                            _stream(torch)))
                hw = [(int(t.height), int(t.width)) for t in table]
                return (flat, hw, [int(t.frame_offset) for t in table]), refused
        finally:
            slot["open"] = False

    def decode_many(self, blobs, pool=None):
        """begin() + finish() for one list of JPEG byte strings."""
        return self.finish(self.begin(blobs, pool))


class _EncodeBatch:
    """A batch between JpegEncoder.begin() and finish(): its pinned slot, its table and what the launches still read."""
    __slots__ = ("slot", "table", "n", "codes", "keep", "done")


class JpegEncoder:
    """One GPU's encoder.  Two pinned buffers in rotation, as JpegDecoder's: begin() uploads the table (and frames given as host
    arrays: ONE pinned upload), enqueues the two launches and the download of the coefficients on the current stream; finish()
    waits for that download and writes the files on the host -- on `pool` (a concurrent.futures executor) when given.  At most
    two batches may be between begin() and finish().  Not thread-safe itself (the emit jobs are)."""
    SAMPLINGS = {"420": SSD_JPEG_SAMPLING_420, "444": SSD_JPEG_SAMPLING_444}

    def __init__(self, device=0):
        torch = _torch()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self._slots = [{"pin": None, "ev": None, "open": False} for _ in range(2)]
        self._turn = 0

    def _frames(self, frames):
        """-> (flat device tensor or None, host arrays or None, [(H, W)...], byte offsets or None)."""
        torch = _torch()
        if isinstance(frames, tuple) and len(frames) == 3 and torch.is_tensor(frames[0]):
            flat, hw, offsets = frames                  # JpegDecoder's form: the frames stay where they are
            if flat.device != self.device or flat.dtype != torch.uint8 or not flat.is_contiguous() or len(hw) != len(offsets):
                raise ValueError("JpegEncoder: (flat, hw, offsets) must be a contiguous uint8 tensor on %s and two lists of one length" % self.device)
            for (h, w), o in zip(hw, offsets):
                if o < 0 or o + 3 * h * w > flat.numel():
                    raise ValueError("JpegEncoder: a frame of (flat, hw, offsets) lies outside flat")
            return flat.reshape(-1), None, [(int(h), int(w)) for h, w in hw], [int(o) for o in offsets]
        frames = list(frames)
        for f in frames:
            if f.ndim != 3 or f.shape[2] != 3 or f.dtype not in (torch.uint8, np.uint8) or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError("JpegEncoder: every frame must be uint8 [H, W, 3]")
        hw = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        on_device = [torch.is_tensor(f) and f.device == self.device for f in frames]
        if frames and all(on_device):
            flat = torch.cat([f.reshape(-1) for f in frames]) if len(frames) > 1 else frames[0].contiguous().reshape(-1)
            return flat, None, hw, [int(o) for o in np.cumsum([0] + [3 * h * w for h, w in hw[:-1]])]
        if any(on_device):
            raise ValueError("JpegEncoder: frames must be all on %s or all on the host" % self.device)
        return None, [np.ascontiguousarray(f.numpy() if torch.is_tensor(f) else f) for f in frames], hw, None

    def _per_frame(self, n, quality, sampling):
        """-> [(sampling code, quality)] * n from scalars or per-frame sequences."""
        qs = [quality] * n if np.ndim(quality) == 0 else list(quality)
        ss = [sampling] * n if isinstance(sampling, str) or np.ndim(sampling) == 0 else list(sampling)
        if len(qs) != n or len(ss) != n:
            raise ValueError("JpegEncoder: quality and sampling must be one value or one per frame")
        for q, smp in zip(qs, ss):
            if str(smp) not in self.SAMPLINGS:
                raise ValueError("JpegEncoder: sampling must be '420' or '444', not %r" % (smp,))
            if not isinstance(q, (int, np.integer)) or not 1 <= q <= 100:
                raise ValueError("JpegEncoder: quality must be an integer in [1, 100], not %r" % (q,))
        return [(self.SAMPLINGS[str(smp)], int(q)) for q, smp in zip(qs, ss)]

    def begin(self, frames, quality=75, sampling="420"):
        """Enqueues a batch on the current stream and returns at once.  `frames`: uint8 [H, W, 3] tensors on this GPU, or host
        arrays (staged through one pinned upload), or JpegDecoder's (flat, hw, offsets).  `quality` and `sampling`: one value
        for the batch, or one per frame."""
        torch = _torch()
        flat, host, hw, offsets = self._frames(frames)
        codes = self._per_frame(len(hw), quality, sampling)
        slot = self._slots[self._turn]
        if slot["open"]:
            raise RuntimeError("JpegEncoder: two batches are already between begin() and finish()")
        self._turn ^= 1
        b = _EncodeBatch()
        b.slot, b.n, b.codes, b.keep, b.done = slot, len(hw), codes, None, False
        n = b.n
        table = (SsdJpegEncodeImage * max(n, 1))()
        totals = (ctypes.c_int64 * 4)()
        rows = np.asarray([(h, w, s, q) for (h, w), (s, q) in zip(hw, codes)], np.int32).reshape(-1, 4)
        rc = lib().ssd_jpeg_encode_plan(rows.ctypes.data, n, table, totals)
        if rc != 0:
            raise SsdError("ssd_jpeg_encode_plan: status %d (a height or width outside [1, 65535]?)" % rc)
        b.table = table
        if n == 0:
            return b
        # the slot: the coefficients come down to its front; the table and the host frames go up from behind them
        table_at = _up16(2 * totals[0])
        frames_at = _up16(table_at + ctypes.sizeof(table))
        need = frames_at + (int(totals[2]) if host is not None else 0)
        if slot["ev"] is not None:
            slot["ev"].synchronize()                    # the copies that last used this buffer
        if slot["pin"] is None or slot["pin"].numel() < need:
            cap = 1 << 20
            while cap < need:
                cap <<= 1
            slot["pin"] = torch.empty((cap,), dtype=torch.uint8).pin_memory()
        slot["open"] = True
        pin = slot["pin"]
        if host is not None:
            view = pin.numpy()
            for t, f in zip(table, host):
                view[frames_at + t.frame_offset:frames_at + t.frame_offset + f.size] = f.reshape(-1)
        else:
            for t, o in zip(table, offsets):
                t.frame_offset = o
        ctypes.memmove(pin.data_ptr() + table_at, table, ctypes.sizeof(table))
        with torch.cuda.device(self.device):
            up = torch.empty((need - table_at,), dtype=torch.uint8, device=self.device)
            up.copy_(pin[table_at:need], non_blocking=True)
            if host is not None:
                flat = up[frames_at - table_at:]
            ws = torch.empty((max(int(totals[1]), 16),), dtype=torch.uint8, device=self.device)
            coef = torch.empty((2 * int(totals[0]),), dtype=torch.uint8, device=self.device)
            check(lib().ssd_jpeg_encode(table, _ptr(up), n, _ptr(flat), _ptr(ws), _ptr(coef), _stream(torch)))
            pin[:coef.numel()].copy_(coef, non_blocking=True)
            if slot["ev"] is None:
                slot["ev"] = torch.cuda.Event()
            slot["ev"].record()
        b.keep = (up, flat, ws, coef)
        return b

    def finish(self, b, pool=None):
        """-> [bytes] of the batch's frames in input order."""
        if b.done:
            raise RuntimeError("JpegEncoder: finish() twice")
        b.done = True
        if b.n == 0:
            return []
        slot = b.slot
        try:
            slot["ev"].synchronize()
            base = slot["pin"].data_ptr()
            bound, emit = lib().ssd_jpeg_emit_bound, lib().ssd_jpeg_emit

            def job(k):
                t, (sampling, quality) = b.table[k], b.codes[k]
                cap = int(bound(t.height, t.width, sampling))
                out, size = np.empty((cap,), np.uint8), ctypes.c_int64()
                rc = emit(base + 2 * t.coef_offset, t.height, t.width, sampling, quality, out.ctypes.data, cap, ctypes.byref(size))
                if rc != 0:
                    raise SsdError("ssd_jpeg_emit: status %d for frame %d" % (rc, k))
                return out[:size.value].tobytes()
            return list(pool.map(job, range(b.n))) if pool is not None else [job(k) for k in range(b.n)]
        finally:
            slot["open"] = False
            b.keep = None

    def encode_many(self, frames, quality=75, sampling="420", pool=None):
        """begin() + finish() for one list of frames -> [bytes], each what PIL's save(format="jpeg", quality=, subsampling=) of
        that frame writes."""
        return self.finish(self.begin(frames, quality, sampling), pool)
