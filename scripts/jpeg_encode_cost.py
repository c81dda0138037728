"""What encoding JPEGs on the GPU costs, part by part, on 32-image batches of 480 x 640 frames, 4:2:0, quality 75:

    python scripts/jpeg_encode_cost.py [--batches 6] [--rounds 3] [--log profiles/jpeg_encode_cost.log]

  per image    PIL's save on one core; ssd_jpeg_emit on one core (from the device stage's coefficients in pinned memory).
  per batch    ssd_jpeg_encode's two launches (HIP events); the download of the batch's coefficients (HIP events).
`--rounds` rounds in ONE process, the four parts alternating, the median of every measurement.  Every file the route writes is
compared with PIL's.  There is no speed gate: no ratio was promised in advance, the log says what was measured, whichever way
it comes out."""
import argparse
import ctypes
import io
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=6)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np            # noqa: E402
import torch                  # noqa: E402
import ssd_amd                # noqa: E402
from PIL import Image         # noqa: E402
from ssd_amd._lib import SsdJpegEncodeImage, lib   # noqa: E402

H, W, B, QUALITY, SAMPLING = 480, 640, 32, 75, 420
med = lambda xs: float(np.median(xs))


def frames(seed):
    """scripts/jpeg_cost.py's scenes: smooth with a little texture, compressing like photographs."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for k in range(B):
        base = np.stack([127 + 100 * np.sin(xx / (20 + 3 * c) + k + seed) * np.cos(yy / (25 + 2 * c)) for c in range(3)], -1)
        out.append(np.clip(base + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def pil_save(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="jpeg")
    return buf.getvalue()


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    L = lib()
    say("device: %s" % torch.cuda.get_device_name(0))
    say("%d batches of %d frames %d x %d, 4:2:0, quality %d, %d rounds" % (args.batches, B, H, W, QUALITY, args.rounds))
    batches = [frames(s) for s in range(args.batches)]
    rows = np.asarray([(H, W, SAMPLING, QUALITY)] * B, np.int32)
    table, totals = (SsdJpegEncodeImage * B)(), (ctypes.c_int64 * 4)()
    assert L.ssd_jpeg_encode_plan(rows.ctypes.data, B, table, totals) == 0
    dev_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    ws = torch.empty((int(totals[1]),), dtype=torch.uint8, device="cuda:0")
    coef = torch.empty((2 * int(totals[0]),), dtype=torch.uint8, device="cuda:0")
    pin = torch.empty((2 * int(totals[0]),), dtype=torch.uint8).pin_memory()
    bound = int(L.ssd_jpeg_emit_bound(H, W, SAMPLING))
    out, size = np.empty(bound, np.uint8), ctypes.c_int64()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t_pil, t_emit, t_k, t_down, sizes = [], [], [], [], []
    for r in range(args.rounds):
        for batch in (batches if r % 2 == 0 else batches[::-1]):
            flat = np.zeros(int(totals[2]), np.uint8)
            for t, f in zip(table, batch):
                flat[t.frame_offset:t.frame_offset + f.size] = f.reshape(-1)
            dev = torch.from_numpy(flat).cuda()
            want = []
            for f in batch:
                t0 = time.perf_counter()
                want.append(pil_save(f))
                t_pil.append(time.perf_counter() - t0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for rep in range(2):                                    # (the second repetition is the timed one)
                torch.cuda.synchronize()
                ev[0].record()
                ssd_amd._lib.check(L.ssd_jpeg_encode(table, dev_table.data_ptr(), B, dev.data_ptr(), ws.data_ptr(), coef.data_ptr(), stream))
                ev[1].record()
                pin.copy_(coef, non_blocking=True)
                ev[2].record()
                torch.cuda.synchronize()
            t_k.append(ev[0].elapsed_time(ev[1]))
            t_down.append(ev[1].elapsed_time(ev[2]))
            for t, w in zip(table, want):
                t0 = time.perf_counter()
                rc = L.ssd_jpeg_emit(pin.data_ptr() + 2 * t.coef_offset, H, W, SAMPLING, QUALITY, out.ctypes.data, bound, ctypes.byref(size))
                t_emit.append(time.perf_counter() - t0)
                assert rc == 0 and out[:size.value].tobytes() == w, "a file differs from PIL's"
                sizes.append(size.value)
    mb = 2 * totals[0] / 1e6
    say("per image, one core:  PIL save %.2f ms   ssd_jpeg_emit %.2f ms   (medians over %d files of %.0f KB)"
        % (med(t_pil) * 1e3, med(t_emit) * 1e3, len(t_pil), med(sizes) / 1024))
    say("per %d-image batch (HIP events, medians over %d batches): the two launches %.3f ms; download of %.1f MB of coefficients %.3f ms = %.1f GB/s"
        % (B, len(t_k), med(t_k), mb, med(t_down), mb / med(t_down)))
    say("per image: the two launches %.4f ms, download %.3f ms, ssd_jpeg_emit %.2f ms on one core; PIL save %.2f ms on one core"
        % (med(t_k) / B, med(t_down) / B, med(t_emit) * 1e3, med(t_pil) * 1e3))
    say("every file equals PIL's byte for byte")
    say("not measured: the upload of host frames, encode_many end to end with a thread pool, other sizes, samplings and qualities")
    say("no ratio was promised in advance, this is what was measured")
    log = args.log or os.path.join(ROOT, "profiles", "jpeg_encode_cost.log")
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
