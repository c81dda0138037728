"""The trainable detection head: detector/box_predictor.py's RetinaNetBoxPredictor in TRAIN mode on this project's own
kernels (include/ssd_hip.h, "the TRAIN head").

    TrainPipeline -> Engine (frozen backbone + FPN, retained p3 .. p7) -> TrainableBoxPredictor -> differentiable_loss
                  -> backward (HIP) -> TrainStep -> checkpoint -> Detector / evaluation

The ops (conv3x3_same, batch_norm_relu) and the variable loading (ReferenceVariables) are train_ops.py's; this file keeps the
head's initialiser rule and its graph.  Freezing the backbone and the FPN is a MODE of this project, not parity with the
reference, which runs every batch norm of the graph on batch statistics in TRAIN mode.
"""
import math

import numpy as np
import torch

from .train_ops import ReferenceVariables, conv3x3_same

MIN_LEVEL = 3                   # detector/constants.py
NUM_ANCHORS_PER_LOCATION = 6
TOWER_DEPTH = 4


def head_variable_shapes(params):
    """The head's subset of variables.variable_shapes(params): box_net/* and class_net/*, statistics included."""
    from .variables import variable_shapes
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("box_net/") or k.startswith("class_net/")}


class TrainableBoxPredictor(ReferenceVariables):
    """RetinaNetBoxPredictor(is_training, num_classes) (box_predictor.py:34-155) as a torch.nn.Module on the HIP kernels.

    params   the model config (num_classes, backbone, depth_multiplier: config.load_config)
    weights  {reference variable name: float32 array in TF layout}, e.g. load_ckpt_weights / synthetic_weights output; only
             box_net/* and class_net/* are read.  A `class_net/logits` whose width is not 6 * num_classes (a new class list) is
             re-drawn with the reference's initialiser: normal(0, 0.01) from `seed`, bias -log(99).
    forward([p3 .. p7], NHWC) -> encoded_boxes [B,N,4], class_predictions [B,N,num_classes] in the anchor order of
    reshape_and_concatenate (:67-104).  .train(): batch statistics, moving statistics move; .eval(): the engine's inference form.
    named_variables() / statistics() are what TrainStep(named_variables(), config, statistics(), layout="tf", params=params) takes."""

    def __init__(self, params, weights, device=None, seed=0):
        def initial(name, shape, rng):
            if name.startswith("class_net/logits/"):
                return rng.normal(0.0, 0.01, shape) if name.endswith("kernel") else np.full(shape, -math.log(99.0))
            if weights.get(name) is None:
                raise KeyError("weights has no variable %r" % name)
        super().__init__(head_variable_shapes(params), weights, initial, device, seed)
        self.params = dict(params)
        self.num_classes = int(params["num_classes"])

    def _net(self, net, last, features):
        n = len(features)
        x = list(features)
        for i in range(TOWER_DEPTH):
            x = conv3x3_same(x, self.variable("%s/conv3x3_%d/kernel" % (net, i)))
            bn = ["%s/batch_norm_%d_for_level_%d" % (net, i, MIN_LEVEL + l) for l in range(n)]
            x = self.batch_norm_relu(x, bn)
        return conv3x3_same(x, self.variable("%s/%s/kernel" % (net, last)), self.variable("%s/%s/bias" % (net, last)))

    def forward(self, image_features):
        feats = list(image_features)
        if not 1 <= len(feats) <= 5:
            raise ValueError("image_features: the pyramid levels p3 .. (at most five)")
        boxes = self._net("box_net", "encoded_boxes", feats)
        logits = self._net("class_net", "logits", feats)
        B = feats[0].shape[0]
        encoded = torch.cat([y.reshape(B, -1, 4) for y in boxes], dim=1)
        classes = torch.cat([y.reshape(B, -1, self.num_classes) for y in logits], dim=1)
        return encoded, classes
