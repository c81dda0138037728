"""What the GPU paths of the evaluation metrics share around their entry points (include/ssd_hip.h: "the COCO box matching", "the
COCO accumulation", "the COCO rows", "the VOC-style metric"): the device a caller names, the stream pointer, the upload of a numpy
array and the timing of a call's parts.  coco_match, coco_accumulate, coco_rows and voc_match import this module inside their GPU
functions only: packing and the host paths keep needing numpy alone."""
import time

import numpy as np
import torch

from .train_calls import stream  # noqa: F401  (the current torch stream as the entry points' `void *stream`: ONE definition)


def device_of(device):
    """A CUDA device index or torch.device -> the torch.device with its index filled in; ValueError for anything but a GPU."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device must be a GPU (a CUDA device index or torch.device): the host loop is evaluate(device=None)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def uploader(dev, what=None, contiguous=False, as_bytes=False):
    """-> up(x, as_bytes=as_bytes) bound to the GPU `dev`.  A numpy array is made contiguous, with as_bytes viewed as flat uint8
    (structured rows, uint16 words), and copied to `dev`.  A tensor must already live there (ValueError '<what> live on ..., not
    on ...') and is returned as it is, through .contiguous() only if `contiguous`."""
    def up(x, as_bytes=as_bytes):
        if isinstance(x, torch.Tensor):
            if x.device != dev:
                raise ValueError("%s live on %s, not on %s" % (what, x.device, dev))
            return x.contiguous() if contiguous else x
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.reshape(-1).view(np.uint8) if as_bytes else x).to(dev)
    return up


class Timer:
    """The clock of a call that takes `timings`: the host clock once the uploads are done, HIP events round the launches.  The call
    decides its own keys.  Off (timings is None), every method returns None at once: no event, no synchronisation."""

    def __init__(self, dev, on):
        self.dev, self.on = dev, on

    def uploaded(self):
        """Waits for the device's current stream, then reads the host clock: the end of 'upload'."""
        if self.on:
            torch.cuda.current_stream(self.dev).synchronize()
            return time.perf_counter()

    def mark(self):
        """An event recorded on the current stream."""
        if self.on:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

    def seconds(self, a, b):
        """Waits for mark b -> the seconds between the marks a and b."""
        if self.on:
            b.synchronize()
            return a.elapsed_time(b) * 1e-3
