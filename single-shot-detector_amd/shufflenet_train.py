"""The trainable ShuffleNet-v2 backbone: detector/backbones/shufflenet_v2.py in TRAIN mode on this project's own kernels
(include/ssd_hip.h, "the TRAIN ShuffleNet").

    TrainPipeline -> TrainableShuffleNet -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward (HIP)
                  -> TrainStep over the three modules' variables (frozen = Conv1) -> checkpoint -> Detector / evaluation

The first convolution -- frozen by default or trained, from uint8 or float32 frames -- is backbone_train.TrainableBackbone's, shared
with TrainableMobileNet, and with it the MODE of this project that is not parity with the reference: BY DEFAULT
Conv1 stays FROZEN and runs in the engine's inference form (ssd.first_conv on its moving statistics).  This file adds the max pool
behind Conv1 (ssd.maxpool3x3s2 with Conv1 frozen, maxpool3x3s2_train with train_first=True, the reference's recipe), the channel
shuffle, and the three stages and Conv5 -- 55 convolutions, each followed by a batch norm, the depthwise ones without an activation --,
which run on batch statistics with all their variables training.
The ops (depthwise_conv, pointwise_conv, concat_shuffle_split, concat_channels, maxpool3x3s2_train) are train_ops.py's; this file keeps
the unit table and the graph.
"""
import torch

from .backbone_train import TrainableBackbone
from .train_ops import concat_channels, concat_shuffle_split, depthwise_conv, maxpool3x3s2_train, pointwise_conv
from .variables import SHUFFLENET_DEPTHS

STAGES = ((2, 4), (3, 8), (4, 4))                   # (stage, units): shufflenet_v2.py:56-66


def shufflenet_variable_shapes(params):
    """The backbone's subset of variables.variable_shapes(params): ShuffleNetV2/*, Conv1 and statistics included."""
    from .variables import variable_shapes
    if params.get("backbone") != "shufflenet":
        raise ValueError("shufflenet_variable_shapes: the config's backbone is %r" % (params.get("backbone"),))
    if float(params["depth_multiplier"]) not in SHUFFLENET_DEPTHS:
        raise ValueError("shufflenet_variable_shapes: depth_multiplier must be one of %s" % sorted(SHUFFLENET_DEPTHS))
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("ShuffleNetV2/")}


class TrainableShuffleNet(TrainableBackbone):
    """shufflenet_v2(images, is_training, depth_multiplier) (shufflenet_v2.py:7-137) as a torch.nn.Module on the HIP kernels, with
    Conv1 frozen by default.

    params   the model config (backbone "shufflenet", depth_multiplier 0.5, 1.0 or 1.5; 2.0 is refused: Conv5 has 2048 channels and
             the batch norm takes at most 1024)
    weights  {reference variable name: float32 array in TF layout}; every ShuffleNetV2/* variable must be there (a missing one is a
             KeyError, not a draw)
    forward(images uint8 or float32 [B,H,W,3] on the GPU, H and W multiples of 32) -> [c3, c4, c5] NHWC float32: Stage2, Stage3 and Conv5.
    .train(): all 56 batch norms (55 with Conv1 frozen) on batch statistics, their moving statistics move; .eval(): the engine's c3,
    c4, c5 bit for bit.  named_variables() / statistics() hold 165 + 110 variables and frozen_variables() the 5 Conv1 arrays for
    TrainStep(..., frozen=backbone.frozen_variables()); with train_first=True 168 + 112 and {}.  keep_features=True keeps the
    post-batch-norm tensor of every layer of the last forward in .features under its scope name (without the "ShuffleNetV2/" prefix
    and the "/batch_norm" suffix; "Conv1" with train_first only), plus "MaxPool", "Stage2" .. "Stage4" and "Conv5" (detached).
    float32 frames are the batches TrainPipeline yields, in [0, 1] (pixel value 2x - 1): first_conv_train_float in
    place of first_conv_train; with Conv1 frozen the raw float convolution on the frozen kernel, the inference batch norm + ReLU and
    the inference max pool.  On frames u * (1 / 255) every result has the bits of the uint8 frames u."""

    FIRST, BN_LEAF, ACT = "ShuffleNetV2/Conv1", "batch_norm", "relu"
    SIZE_MULTIPLE, SIZE_MESSAGE = 32, "images: height and width must be multiples of 32 (the network's stride)"

    def __init__(self, params, weights, device=None, seed=0, keep_features=False, train_first=False):
        if params.get("backbone") != "shufflenet":
            raise ValueError("TrainableShuffleNet: the config's backbone is %r" % (params.get("backbone"),))
        if float(params["depth_multiplier"]) not in (0.5, 1.0, 1.5):
            raise ValueError("TrainableShuffleNet: depth_multiplier must be 0.5, 1.0 or 1.5 (2.0: Conv5 has 2048 channels, the batch norm "
                             "takes at most 1024)")
        super().__init__(shufflenet_variable_shapes(params), params, weights, device, seed, keep_features, train_first)
        self._feats = {}

    def first_conv(self, images):
        """Conv1 and MaxPool: TrainableBackbone.first_conv (the convolution, its batch norm and ReLU), then the 3x3 stride-2 max
        pool -- with its gradient with train_first, the inference max pool with Conv1 frozen."""
        from . import ssd
        self._feats = {}
        x = super().first_conv(images)
        if self.train_first:
            self._keep("Conv1", x)
            x = maxpool3x3s2_train(x)
        else:
            with torch.cuda.device(images.device):
                x = ssd.maxpool3x3s2(x)
        self._keep("MaxPool", x)
        return x

    def _keep(self, name, x):
        if self.keep_features:
            self._feats[name] = x.detach()

    def _conv(self, x, scope):
        x = self._bn(pointwise_conv(x, self.variable("ShuffleNetV2/" + scope + "/weights")), "ShuffleNetV2/" + scope)
        self._keep(scope, x)
        return x

    def _dw(self, x, scope, stride):
        # depthwise_conv(..., activation_fn=None): a batch norm and nothing after it (shufflenet_v2.py:121,131,135)
        x = self._bn(depthwise_conv(x, self.variable("ShuffleNetV2/" + scope + "/depthwise_weights"), stride), "ShuffleNetV2/" + scope, act="none")
        self._keep(scope, x)
        return x

    def _stage(self, x, stage, units):
        u = "Stage%d/unit_1" % stage                             # basic_unit_with_downsampling (:126-137)
        y = self._conv(x, u + "/conv1x1_before")
        y = self._dw(y, u + "/depthwise", 2)
        y = self._conv(y, u + "/conv1x1_after")
        x = self._dw(x, u + "/second_branch/depthwise", 2)
        x = self._conv(x, u + "/second_branch/conv1x1_after")
        for j in range(2, units + 1):                            # concat_shuffle_split + basic_unit (:79-91, :118-123)
            x, y = concat_shuffle_split(x, y)
            u = "Stage%d/unit_%d" % (stage, j)
            x = self._conv(x, u + "/conv1x1_before")
            x = self._dw(x, u + "/depthwise", 1)
            x = self._conv(x, u + "/conv1x1_after")
        x = concat_channels(x, y)
        self._keep("Stage%d" % stage, x)
        return x

    def body(self, x):
        """Stage2 .. Stage4 and Conv5 on MaxPool's output [B,H/4,W/4,24] -> [c3, c4, c5]."""
        outs = []
        for stage, units in STAGES:
            x = self._stage(x, stage, units)
            outs.append(x)
        outs[2] = self._conv(x, "Conv5")
        self.features = self._feats
        return outs

    def forward(self, images):
        return self.body(self.first_conv(images))
