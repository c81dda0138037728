"""Baseline JPEG bytes -> uint8 RGB frames in device memory, laid out as Engine.forward_mixed takes them (include/ssd_hip.h, block
"the JPEG decoder"): the marker structure and the Huffman decoding on the host (ssd_jpeg_info_read, ssd_jpeg_entropy: plain C,
called through ctypes, which releases the interpreter lock -- a caller's thread pool runs them in parallel), everything behind the
quantised coefficients in two launches on the GPU (ssd_jpeg_decode).  The frames are bit for bit what
PIL.Image.open(...).convert("RGB") gives; a file the decoder does not take (progressive, CMYK, other samplings, a damaged stream,
..) is REFUSED by index and stays with the caller's own reader -- nothing is decoded some other way behind the caller's back.

    dec = JpegDecoder(0)
    (flat, hw, offsets), refused = dec.decode_many(list_of_bytes)
    engine.forward_mixed((flat, hw_of_one_network_shape, offsets_of_them), records)
"""
import ctypes

from ._lib import SSD_ERR_INVALID, SSD_ERR_UNSUPPORTED, SsdJpegImage, SsdJpegInfo, check, lib
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
