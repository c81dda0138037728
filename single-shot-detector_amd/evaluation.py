"""train.py's evaluation (train.py:61-65: EvalSpec over the validation shards, model.py:79-104 in mode EVAL) without
TensorFlow: the validation loss of a checkpoint and the VOC-style AP of metrics.py.

    python -m ssd_amd.evaluation MODEL_PATH --config config.json [--val_dataset DIR] [--use_ema] [--gpu-metric]

EVAL runs at batch 1 (pipeline.py:22-27), so every image is normalised by its OWN matches; `loss` is the mean over
images of total_loss = localization_loss_weight * localization + classification_loss_weight * classification +
regularization (model.py:79-104), what estimator.evaluate reports.  Here the images are grouped by the size the network
sees and run as mixed-size batches (Engine.forward_mixed), the loss kernels (ssd_loss) give the per-image sums, and the
predictions come from the same retained tensors through batch_multiclass_non_max_suppression WITHOUT the division by
box_scaler (model.py divides in PREDICT only): the groundtruth boxes are multiplied by box_scaler instead
(pipeline.py:103-109), and both meet in the padded frame.
"""
import os

import numpy as np

from .coco_eval import Evaluator
from .config import load_loss_config
from .ssd import (AnchorGenerator, batch_multiclass_non_max_suppression, mixed_batches, network_input_size, split_records,
                  ssd_loss, _torch)

_METRIC_NAMES = ("AP", "precision", "recall", "mean_iou_for_TP", "best_threshold", "total_FP", "total_FN")   # metrics.py:84-100


def l2_sum(weights):
    """The sum of tf.nn.l2_loss(K) (= sum(K^2) / 2) over the variables add_weight_decay regularises (model.py:132-145: the
    names containing 'weights' or 'kernel' but not 'depthwise_weights'), in float64."""
    s = 0.0
    for name in sorted(weights):
        if ("weights" in name or "kernel" in name) and "depthwise_weights" not in name:
            k = np.asarray(weights[name], np.float64).reshape(-1)
            s += float(np.dot(k, k)) / 2.0
    return s


def regularization_loss(weights, weight_decay):
    """model.py:80-81: weight_decay * l2_sum(weights), evaluated in float64 and rounded to float32 once."""
    return np.float32(float(weight_decay) * l2_sum(weights))


def total_loss(localization, classification, regularization, loss_config):
    """tf.losses.get_total_loss (model.py:100-104) of one image: each weighted term one fp32 product, their sum in
    float64 rounded once."""
    lw = np.float32(loss_config["localization_loss_weight"]) * np.float32(localization)
    cw = np.float32(loss_config["classification_loss_weight"]) * np.float32(classification)
    return np.float32(float(lw) + float(cw) + float(regularization))


class _Run:
    """The loss + predictions of one mixed-size batch of decoded frames on one engine."""

    def __init__(self, engine):
        self.engine = engine
        self.anchors = {}
        engine.set_option("logits_screen", 0)       # the loss reads every logit: the dense launch, not screen + fill + dense on demand

    def anchors_for(self, shape):
        a = self.anchors.get(shape)
        if a is None:
            gen = AnchorGenerator()
            t = _torch().from_numpy(gen(*shape)).to("cuda:%d" % self.engine.device)
            a = self.anchors[shape] = (t, list(gen.num_anchors_per_feature_map))
        return a

    def __call__(self, frames, gts, loss_config):
        """frames: uint8 arrays [H,W,3] of one network shape; gts: (boxes [n,4] normalised to the frame, labels [n]).
        -> per image (localization, classification, matches) and the predictions (boxes, labels, scores) trimmed to
        num_boxes, boxes in the padded frame."""
        torch = _torch()
        eng, p = self.engine, self.engine.params
        dev = "cuda:%d" % eng.device
        shape = eng.network_shape(frames[0].shape[0], frames[0].shape[1])
        anchors, per_level = self.anchors_for(shape)
        B, N, C = len(frames), int(anchors.shape[0]), int(p["num_classes"])
        eng.forward_mixed([torch.from_numpy(np.require(f, np.uint8, ["C", "W"])).to(dev) for f in frames])
        logits = eng.get_tensor_dev("class_predictions", (B, N, C))
        codes = eng.get_tensor_dev("encoded_boxes", (B, N, 4))
        G = max(1, max(len(g[1]) for g in gts))
        boxes = np.zeros((B, G, 4), np.float32)
        labels = np.zeros((B, G), np.int32)
        num = np.zeros((B,), np.int32)
        scaled = []
        for b, (f, (gb, gl)) in enumerate(zip(frames, gts)):
            bs = network_input_size(f.shape[0], f.shape[1], p["min_dimension"])[2]
            s = np.asarray(gb, np.float32).reshape(-1, 4) * bs                      # pipeline.py:109, float32
            scaled.append(s)
            boxes[b, :len(s)] = s
            labels[b, :len(s)] = gl
            num[b] = len(s)
        _losses, per_image = ssd_loss(logits, codes, anchors, {"boxes": boxes, "labels": labels, "num_boxes": num},
                                      gamma=loss_config["gamma"], alpha=loss_config["alpha"], anchors_per_level=per_level)
        pb, ps, pc, pn = batch_multiclass_non_max_suppression(codes, anchors, logits, p["score_threshold"], p["iou_threshold"],
                                                              p["max_boxes_per_class"], box_scaler=None)
        per_image, pb, ps, pc, pn = (t.cpu().numpy() for t in (per_image, pb, ps, pc, pn))
        out = []
        for b in range(B):
            n = int(pn[b])
            out.append((per_image[b, :3], scaled[b], (pb[b, :n], pc[b, :n], ps[b, :n])))
        return out


def image_losses(per_image_row, regularization, loss_config):
    """(localization, classification, total) of one image at batch 1 from its ssd_loss per_image row."""
    norm = max(np.float32(per_image_row[2]), np.float32(1.0))
    loc = np.float32(per_image_row[0]) / norm
    cls = np.float32(per_image_row[1]) / norm
    return loc, cls, total_loss(loc, cls, regularization, loss_config)


def evaluate(detector, val_dataset, config, max_batch=32, read_workers=None, decode=None, group=None, chunk=256, metric_device=None):
    """estimator.evaluate of train.py:61-65 for `detector` (a Detector) over `val_dataset` (a directory of .tfrecords
    shards, a shard path, or an iterable of (JPEG bytes | uint8 array, boxes [n,4], labels [n])).  config: the
    reference's JSON (path or dict).  Returns {'loss', 'localization_loss', 'classification_loss',
    'regularization_loss'} (means over images) and 'metrics/mAP' -- or the seven 'metrics/*' of metrics.py:84-100 when
    num_classes == 1.  JPEGs are decoded on `read_workers` threads (default min(16, CPUs)).

    `group`: a torch.distributed process group to shard the images over (None: this process does everything).  Every rank
    iterates the whole record stream (bytes only) and decodes and runs only its own round-robin chunks of `chunk` images
    (distributed.ChunkAssignment); per round one all-gather of one fixed-size row per image (the ssd_loss row, the frame size
    and the predictions) follows, and the means and the Evaluator are fed in dataset order on every rank: every rank
    returns the one-process dict, float for float.

    `metric_device`: None computes the metric with coco_eval.Evaluator's host loop; a CUDA device index or torch.device computes it
    on that GPU (voc_match.VocEvaluator: two launches over all images; under `group` every rank on the device it names, as every
    rank runs the host loop): every 'metrics/*' value the same float, except the AP and mAP, whose sums the kernel forms in row
    order -- equal or the adjacent float32."""
    from concurrent.futures import ThreadPoolExecutor
    from . import tfrecords
    from .distributed import ChunkAssignment, read_worker_count
    lc = load_loss_config(config)
    eng = detector.engine
    reg = detector.regularization_loss(lc["weight_decay"])
    if decode is None:
        decode = tfrecords.decode_image
    data = tfrecords.read_dataset(val_dataset) if isinstance(val_dataset, (str, os.PathLike)) else val_dataset
    if metric_device is None:
        evaluator = Evaluator(int(eng.params["num_classes"]))
    else:
        from .voc_match import VocEvaluator
        evaluator = VocEvaluator(int(eng.params["num_classes"]))
    run = _Run(eng)
    sums = np.zeros(4, np.float64)
    count = 0
    workers = read_worker_count(read_workers)
    if group is None:
        world, rank = 1, 0
    else:
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    assign = ChunkAssignment(world, rank, chunk)

    def run_items(items):
        """(frame, boxes, labels) triples -> _Run's per-image results, in the order of `items`."""
        results = [None] * len(items)
        for part in mixed_batches(eng, [frame.shape[:2] for frame, _gb, _gl in items], max_batch):
            with eng.lock:
                res = run([items[i][0] for i in part], [(items[i][1], items[i][2]) for i in part], lc)
            for i, r in zip(part, res):
                results[i] = r
        return results

    def add(result, gl):
        nonlocal count, sums
        row, gt_scaled, (bx, lb, sc) = result
        loc, cls, tot = image_losses(row, reg, lc)
        sums = sums + np.array([float(tot), float(loc), float(cls), float(reg)])
        count += 1
        evaluator.add_image(gt_scaled, gl, bx, lb, sc)

    def flush(items):
        """One round: this rank's chunk of `items` decoded and run, every rank's results exchanged, all fed in dataset order."""
        own = [(f.result(), gb, gl) for f, gb, gl in items[rank * chunk:(rank + 1) * chunk]]
        results = run_items(own)
        if group is not None:
            results = _exchange(eng, own, results, items, group, chunk)
        for result, (_f, _gb, gl) in zip(results, items):
            add(result, gl)

    # round k is images [k * world * chunk, (k + 1) * world * chunk) of the stream: a chunk per rank (world 1: the whole round)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        items = []
        for i, (img, gb, gl) in enumerate(data):
            items.append((pool.submit(decode, img) if assign.mine(i) else None, gb, gl))
            if len(items) == world * chunk:
                flush(items)
                items = []
        if items:
            flush(items)
    if count == 0:
        raise ValueError("the validation dataset is empty")
    means = sums / count
    out = {"loss": float(np.float32(means[0])), "localization_loss": float(np.float32(means[1])),
           "classification_loss": float(np.float32(means[2])), "regularization_loss": float(np.float32(means[3]))}
    m = evaluator.evaluate() if metric_device is None else evaluator.evaluate(device=metric_device)
    if evaluator.num_classes == 1:
        for k in _METRIC_NAMES:
            out["metrics/" + k] = float(np.float32(m[0][k]))
    else:
        out["metrics/mAP"] = float(np.float32(m["mAP"]))
    out["num_images"] = count
    return out


def _exchange(eng, own, results, items, group, chunk):
    """evaluate()'s all-gather of one round over the ranks of `group`: this rank's `results` (of its decoded frames `own`) ->
    every rank's, in the order of the round's `items`.  One row per image: 5 prefix words -- the ssd_loss row (localization
    sum, classification sum, matches: 3 x f32), the frame's height and width -- then the predictions as an ordinary record
    (split_records); one all-gather of [world * chunk, 5 + 6T+1] int32.  The groundtruth boxes are scaled by the frame's
    box_scaler here, as _Run scales them."""
    import torch.distributed as dist
    from .distributed import gather_records
    torch = _torch()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    per = min(chunk, len(items))
    rows = np.zeros((per, 5 + eng.record_words), np.int32)
    boxes, labels, scores, num = split_records(rows[:, 5:])
    for j, ((frame, _gb, _gl), (row, _s, (bx, lb, sc))) in enumerate(zip(own, results)):
        n = len(sc)
        rows[j, 0:3] = np.asarray(row[:3], np.float32).view(np.int32)
        rows[j, 3:5] = frame.shape[:2]
        boxes[j, :n], labels[j, :n], scores[j, :n], num[j] = bx, lb, sc, n
    dev = torch.device("cuda", eng.device) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    got = gather_records(torch.from_numpy(rows).to(dev), group).cpu().numpy()
    boxes, labels, scores, num = split_records(got[:, 5:])
    out = []
    for q, (_f, gb, _gl) in enumerate(items):
        r, j = divmod(q, chunk)
        i, n = r * per + j, int(num[r * per + j])
        bs = network_input_size(int(got[i, 3]), int(got[i, 4]), eng.params["min_dimension"])[2]
        out.append((got[i, 0:3].view(np.float32), np.asarray(gb, np.float32).reshape(-1, 4) * bs,
                    (boxes[i, :n], labels[i, :n], scores[i, :n])))
    return out


def main(argv=None):
    import argparse
    import json
    import sys
    from .detector import Detector
    ap = argparse.ArgumentParser(description="train.py's evaluation of a checkpoint: validation loss and AP")
    ap.add_argument("model_path", help="checkpoint prefix / model_dir / frozen graph / .npz")
    ap.add_argument("--config", required=True, help="the reference's JSON config")
    ap.add_argument("--val_dataset", default=None, help="directory of .tfrecords shards (default: the config's val_dataset)")
    ap.add_argument("--use_ema", action="store_true", help="the moving averages, as RestoreMovingAverageHook restores them")
    ap.add_argument("--max_batch", type=int, default=32)
    ap.add_argument("--gpus", type=int, default=1,
                    help="processes to shard the images over: N > 1 starts torch.distributed.run with N ranks as a child process "
                         "(rank r on device LOCAL_RANK %% device_count; RCCL only when every rank has a device of its own, else "
                         "gloo); inside such a launch the collective path runs, also at N = 1")
    ap.add_argument("--gpu-metric", "--gpu_metric", dest="gpu_metric", action="store_true",
                    help="the AP on the GPU (voc_match.VocEvaluator) instead of coco_eval.Evaluator's host loop")
    a = ap.parse_args(argv)
    if a.gpus < 1:
        ap.error("--gpus must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from .distributed import launch_local
        # nothing here has touched the GPU yet; the child runs this module again, once per rank
        sys.exit(launch_local(a.gpus, "ssd_amd.evaluation", sys.argv[1:] if argv is None else list(argv)))
    val = a.val_dataset or json.load(open(a.config))["val_dataset"]
    if "WORLD_SIZE" not in os.environ:
        with Detector(a.model_path, config=a.config, use_ema=a.use_ema) as det:
            print(json.dumps(evaluate(det, val, a.config, max_batch=a.max_batch, metric_device=det.engine.device if a.gpu_metric else None),
                             sort_keys=True))
        return
    import torch.distributed as dist
    from .distributed import init_node_process_group
    if a.gpus != int(os.environ["WORLD_SIZE"]):
        raise SystemExit("--gpus (%d) != WORLD_SIZE (%s)" % (a.gpus, os.environ["WORLD_SIZE"]))
    device, _backend = init_node_process_group()
    try:
        with Detector(a.model_path, config=a.config, use_ema=a.use_ema, visible_device_list=str(device)) as det:
            res = evaluate(det, val, a.config, max_batch=a.max_batch, group=dist.group.WORLD,
                           metric_device=det.engine.device if a.gpu_metric else None)
        if dist.get_rank() == 0:
            print(json.dumps(res, sort_keys=True), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
