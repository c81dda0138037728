"""A float32 numpy restatement of ssd_augment (csrc/augment.hip; semantics in include/ssd_hip.h, block "the TRAIN input
pipeline"): every step one float32 op, as the kernel does it, so that the kernel must match it bit for bit.  Test
infrastructure only."""
import numpy as np

f32 = np.float32
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counters, key):
    """Philox4x32-10 on the counters (c, 0, 0, 0) for every c of `counters` with the 64-bit `key` (word 0 = the low half)
    -> uint32 [n, 4]."""
    c0 = np.asarray(counters, np.uint64).reshape(-1) & M32
    c1 = np.zeros_like(c0)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = np.uint64(int(key) & 0xFFFFFFFF), np.uint64(int(key) >> 32)
    for i in range(10):
        if i:
            k0 = (k0 + np.uint64(0x9E3779B9)) & M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & M32
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def uint_to_unit(words):
    """TF's Uint32ToFloat: as_float(0x3f800000 | (w & 0x7fffff)) - 1."""
    w = (np.asarray(words, np.uint32) & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)
    return w.view(np.float32) - f32(1)


def source_index(out, crop_start, crop_len):
    """crop_start + min(floor(dst * (crop_len / out)), crop_len - 1), the scale one correctly rounded float32 division."""
    scale = f32(crop_len) / f32(out)
    v = np.floor(np.arange(out).astype(np.float32) * scale).astype(np.int64)
    return crop_start + np.minimum(v, crop_len - 1)


def augment(frame, p, out_h, out_w, channels_first=False):
    """One image: frame uint8 [H, W, 3], p an ssd_augment_params row (augment.PARAMS_DTYPE; offset ignored) -> float32
    [out_h, out_w, 3] (or [3, out_h, out_w])."""
    frame = np.asarray(frame, np.uint8)
    assert frame.shape == (int(p["height"]), int(p["width"]), 3)
    sy = source_index(out_h, int(p["crop_y"]), int(p["crop_h"]))
    sx = source_index(out_w, int(p["crop_x"]), int(p["crop_w"]))
    v = frame[sy][:, sx].astype(np.float32) * f32(1.0 / 255.0)
    flags = int(p["flags"])
    if flags & 1:
        v = np.clip(v + np.asarray(p["color_offset"], np.float32), f32(0), f32(1))
    if flags & 2:
        g = (v[..., 0] * f32(0.2989) + v[..., 1] * f32(0.5870)) + v[..., 2] * f32(0.1140)
        v = np.stack([g, g, g], axis=-1)
    if flags & 4:
        ctr = (np.arange(out_h, dtype=np.uint64)[:, None] * np.uint64(out_w) + np.arange(out_w, dtype=np.uint64)[None, :])
        u = uint_to_unit(philox4x32_10(ctr.reshape(-1), int(p["philox_key"]))[:, :3]).reshape(out_h, out_w, 3)
        v = np.clip(v * (u * f32(p["scale_range"]) + f32(p["scale_min"])), f32(0), f32(1))
    if flags & 8:
        v = v[:, ::-1]
    v = np.ascontiguousarray(v, np.float32)
    return np.ascontiguousarray(v.transpose(2, 0, 1)) if channels_first else v
