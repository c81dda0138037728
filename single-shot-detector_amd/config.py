"""The reference's JSON config surface (config_mobilenet.json / config_shufflenet.json).

Only the keys the inference graph consumes are used (model.py:22-30,46,57-61;
create_pb.py:24); training keys are accepted and ignored so the reference's files load
unmodified.
"""
import json
import math

INFERENCE_KEYS = ("backbone", "depth_multiplier", "num_classes", "score_threshold",
                  "iou_threshold", "max_boxes_per_class", "min_dimension")

_DEFAULTS = {"min_dimension": 640}      # create_pb.py:24 MIN_DIMENSION


def load_config(path_or_dict):
    """Returns a dict with exactly INFERENCE_KEYS.  Raises KeyError / ValueError like the
    reference would fail on a malformed config (model.py indexes params[...] directly)."""
    if isinstance(path_or_dict, dict):
        raw = dict(path_or_dict)
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    out = {}
    for k in INFERENCE_KEYS:
        if k in raw:
            out[k] = raw[k]
        elif k in _DEFAULTS:
            out[k] = _DEFAULTS[k]
        else:
            raise KeyError("config is missing the key %r" % k)
    if out["backbone"] not in ("mobilenet", "shufflenet"):
        raise ValueError("backbone must be 'mobilenet' or 'shufflenet' (model.py:22-30)")
    out["depth_multiplier"] = float(out["depth_multiplier"])
    out["num_classes"] = int(out["num_classes"])
    out["score_threshold"] = float(out["score_threshold"])
    out["iou_threshold"] = float(out["iou_threshold"])
    out["max_boxes_per_class"] = int(out["max_boxes_per_class"])
    out["min_dimension"] = int(out["min_dimension"])
    return out


LOSS_KEYS = ("gamma", "alpha", "localization_loss_weight", "classification_loss_weight", "weight_decay")


def load_loss_config(path_or_dict):
    """The keys of the reference's JSON config that the EVAL loss reads (model.py:80-104, ssd.py:102-103): a dict with
    exactly LOSS_KEYS as floats.  load_config / INFERENCE_KEYS are unaffected."""
    if isinstance(path_or_dict, dict):
        raw = dict(path_or_dict)
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    missing = [k for k in LOSS_KEYS if k not in raw]
    if missing:
        raise KeyError("config is missing the key %r" % missing[0])
    return {k: float(raw[k]) for k in LOSS_KEYS}


TRAIN_KEYS = ("batch_size", "image_height", "image_width")


def load_train_config(path_or_dict):
    """The keys of the reference's JSON config that the TRAIN input pipeline reads (pipeline.py:28-33): a dict with exactly
    TRAIN_KEYS as ints.  image_height and image_width must be positive multiples of 128 (DIVISOR, pipeline.py:32-33)."""
    if isinstance(path_or_dict, dict):
        raw = dict(path_or_dict)
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    missing = [k for k in TRAIN_KEYS if k not in raw]
    if missing:
        raise KeyError("config is missing the key %r" % missing[0])
    out = {k: int(raw[k]) for k in TRAIN_KEYS}
    if out["batch_size"] < 1:
        raise ValueError("batch_size must be >= 1")
    if min(out["image_height"], out["image_width"]) < 128 or out["image_height"] % 128 or out["image_width"] % 128:
        raise ValueError("image_height and image_width must be positive multiples of 128 (pipeline.py:32-33)")
    return out


OPTIMIZER_KEYS = ("initial_learning_rate", "num_steps", "weight_decay")


def load_optimizer_config(path_or_dict):
    """The keys of the reference's JSON config that the TRAIN update reads (model.py:80-81,108-113): a dict with exactly
    OPTIMIZER_KEYS, initial_learning_rate and weight_decay as floats, num_steps (the cosine decay's decay_steps) as a positive int."""
    if isinstance(path_or_dict, dict):
        raw = dict(path_or_dict)
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    missing = [k for k in OPTIMIZER_KEYS if k not in raw]
    if missing:
        raise KeyError("config is missing the key %r" % missing[0])
    out = {"initial_learning_rate": float(raw["initial_learning_rate"]), "num_steps": int(raw["num_steps"]),
           "weight_decay": float(raw["weight_decay"])}
    if out["num_steps"] < 1:
        raise ValueError("num_steps must be >= 1")
    if not (math.isfinite(out["initial_learning_rate"]) and math.isfinite(out["weight_decay"])):
        raise ValueError("initial_learning_rate and weight_decay must be finite")
    return out


RUN_KEYS = ("model_dir", "train_dataset", "val_dataset", "pretrained_checkpoint")


def load_run_config(path_or_dict):
    """The keys of the reference's JSON config that train.py itself reads (train.py:19,36-50): a dict with exactly RUN_KEYS as
    strings -- where the run lives, its two datasets and the checkpoint whose backbone warm-starts it."""
    if isinstance(path_or_dict, dict):
        raw = dict(path_or_dict)
    else:
        with open(path_or_dict) as f:
            raw = json.load(f)
    missing = [k for k in RUN_KEYS if k not in raw]
    if missing:
        raise KeyError("config is missing the key %r" % missing[0])
    return {k: str(raw[k]) for k in RUN_KEYS}
