"""A stand-in Detector for the sharding tests without a GPU: its engine has the record interface detect_many_sharded uses
(record_words, network_shape, MIXED_MAX, new_records, forward_mixed_host(images, records=...)) and writes, per image, a record that is a
pure function of the image -- a varying number of detections, zero included, scores on both sides of the threshold and
garbage beyond num_boxes."""
import threading

import numpy as np


def record_of(image, T):
    seed = int(image.astype(np.int64).sum()) * 7919 + image.shape[0] * 1009 + image.shape[1]
    rng = np.random.default_rng(seed)
    rec = np.empty(6 * T + 1, np.int32)
    rec[:4 * T] = rng.random(4 * T, dtype=np.float32).view(np.int32)
    rec[4 * T:5 * T] = rng.random(T, dtype=np.float32).view(np.int32)
    rec[5 * T:6 * T] = rng.integers(0, 80, T, dtype=np.int32)
    rec[6 * T] = seed % (T + 1)
    return rec


def filtered(rec, T, score_threshold):
    boxes = rec[:4 * T].view(np.float32).reshape(T, 4)
    scores, labels, n = rec[4 * T:5 * T].view(np.float32), rec[5 * T:6 * T], int(rec[6 * T])
    keep = scores[:n] > score_threshold
    return boxes[:n][keep], labels[:n][keep], scores[:n][keep]


class StubEngine:
    MIXED_MAX = 64
    precision = "f32"
    device = 0

    def __init__(self, T):
        self.T, self.record_words = T, 6 * T + 1
        self.lock = threading.RLock()
        self.batches = []

    def network_shape(self, height, width):
        return (-(-height // 64) * 64, -(-width // 64) * 64)

    def new_records(self, B, dev):
        import torch
        return torch.empty((B, self.record_words), dtype=torch.int32, device=dev)

    def forward_mixed_host(self, images, records):
        import torch
        assert len({self.network_shape(*im.shape[:2]) for im in images}) == 1, "one network shape per batch"
        assert tuple(records.shape) == (len(images), self.record_words) and records.is_contiguous()
        self.batches.append(len(images))
        for b, im in enumerate(images):
            records[b] = torch.from_numpy(record_of(im, self.T))


class StubDetector:
    def __init__(self, T=7):
        self.engine = StubEngine(T)

    def detect_many(self, images, score_threshold=0.1, max_batch=32):
        return [filtered(record_of(np.asarray(im), self.engine.T), self.engine.T, score_threshold) for im in images]

    def __call__(self, image, score_threshold=0.1):
        return self.detect_many([image], score_threshold)[0]


def images(seed, n, sizes=((40, 60), (64, 64), (100, 30), (130, 70), (20, 200))):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, sizes[int(rng.integers(0, len(sizes)))] + (3,), dtype=np.uint8) for _ in range(n)]
