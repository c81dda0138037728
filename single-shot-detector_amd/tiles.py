"""Tiled detection (include/ssd_hip.h, block "tiled detection"): the grid of overlapping tiles over a frame larger than the
network's input, and the two device calls around the forwards of Detector.detect_tiled -- ssd_tile_gather cuts the tiles out of the
frames where they lie, ssd_tile_merge joins the tiles' records (and the whole frame's) by the detector's NMS rule."""
import ctypes

from ._lib import check, lib
from .ssd import _stream

MAX_CANDIDATES = 2048        # SSD_TILE_MAX_CANDIDATES


def overlap_pixels(th, tw, overlap):
    """(oy, ox): the rows and columns two neighbouring tiles share, int(overlap * side)."""
    return int(overlap * th), int(overlap * tw)


def tile_grid(H, W, th, tw, overlap):
    """The grid of a frame [H, W] under tiles [th, tw] that overlap by the fraction `overlap` of a tile side -> (ys, xs), the
    lists of the tiles' top rows and left columns; tile (iy, ix) of frame f has index (f * len(ys) + iy) * len(xs) + ix.  The
    counts and steps are the library's (ssd_tile_grid: a host function, no GPU); ValueError where it refuses -- a frame smaller
    than the tile, a side that is no multiple of 128, an overlap that leaves no step."""
    oy, ox = overlap_pixels(th, tw, overlap)
    g = (ctypes.c_int32 * 4)()
    if lib().ssd_tile_grid(int(H), int(W), int(th), int(tw), oy, ox, g) != 0:
        raise ValueError(lib().ssd_last_error().decode())
    ny, nx, sy, sx = g
    return [min(i * sy, H - th) for i in range(ny)], [min(i * sx, W - tw) for i in range(nx)]


def tile_gather(frames, th, tw, overlap, out=None):
    """frames: uint8 CUDA tensor [F, H, W, 3] -> its tiles, uint8 [F * ny * nx, th, tw, 3] (`out`, or a new tensor); one launch
    on the current stream."""
    import torch
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4 and frames.shape[3] == 3):
        raise TypeError("frames must be a contiguous uint8 CUDA tensor [F, H, W, 3]")
    F, H, W, _ = frames.shape
    ys, xs = tile_grid(H, W, th, tw, overlap)
    n = F * len(ys) * len(xs)
    if out is None:
        out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=frames.device)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, th, tw, 3)):
        raise TypeError("out must be a contiguous uint8 CUDA tensor [%d, %d, %d, 3]" % (n, th, tw))
    oy, ox = overlap_pixels(th, tw, overlap)
    check(lib().ssd_tile_gather(frames.data_ptr(), F, H, W, th, tw, oy, ox, out.data_ptr(), _stream(torch)))
    return out


def tile_merge(tile_records, full_records, frame_shape, th, tw, overlap, num_classes, max_boxes_per_class, iou_threshold, out=None):
    """tile_records: int32 CUDA tensor [F * ny * nx, 6T + 1], full_records: [F, 6T + 1] or None, frame_shape: (F, H, W) -> the
    merged records [F, 6T + 1] (`out`, or a new tensor), boxes normalised to the frame; two launches on the current stream."""
    import torch
    F, H, W = (int(v) for v in frame_shape)
    ys, xs = tile_grid(H, W, th, tw, overlap)
    words = 6 * int(num_classes) * int(max_boxes_per_class) + 1
    if out is None:
        out = torch.empty((F, words), dtype=torch.int32, device=tile_records.device)
    for name, t, rows in (("tile_records", tile_records, F * len(ys) * len(xs)), ("full_records", full_records, F), ("out", out, F)):
        if t is None and name == "full_records":
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (rows, words)):
            raise TypeError("%s must be a contiguous int32 CUDA tensor [%d, %d]" % (name, rows, words))
    oy, ox = overlap_pixels(th, tw, overlap)
    check(lib().ssd_tile_merge(tile_records.data_ptr(), None if full_records is None else full_records.data_ptr(), F, H, W, th, tw, oy, ox,
                               int(num_classes), int(max_boxes_per_class), float(iou_threshold), out.data_ptr(), _stream(torch)))
    return out
