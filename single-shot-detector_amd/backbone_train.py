"""The trainable MobileNet-v1 backbone: detector/backbones/mobilenet_v1.py in TRAIN mode on this project's own kernels
(include/ssd_hip.h, "the TRAIN backbone").

    TrainPipeline -> TrainableMobileNet -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss -> backward (HIP)
                  -> TrainStep over the three modules' variables (frozen = Conv2d_0) -> checkpoint -> Detector / evaluation

train.py:44-50 warm-starts the backbone and then trains it with everything else; this module is that, with one difference that is
a MODE of this project and not parity with the reference: BY DEFAULT Conv2d_0 stays FROZEN.  It runs in the
engine's inference form (ssd.first_conv on its moving statistics); Conv2d_1 .. Conv2d_13 -- 13 depthwise and 13 pointwise layers,
each followed by a batch norm and ReLU6 -- run on batch statistics and all their variables train.  train_first=True (DESIGN.md
4.14) trains Conv2d_0 as well, the reference's recipe: first_conv_train on uint8 frames or first_conv_train_float on the float32
batches TrainPipeline yields, then the batch norm on batch statistics.  The ops (first_conv_train,
first_conv_train_float, depthwise_conv, pointwise_conv, batch_norm_act) and the variable loading
(ReferenceVariables) are train_ops.py's; this file keeps TrainableBackbone -- the first convolution's four routes and the frozen
variables, shared with shufflenet_train.TrainableShuffleNet --, the layer table and the graph.
"""
import numpy as np
import torch

from .train_ops import (BATCH_NORM_EPSILON, ReferenceVariables, batch_norm_act, depthwise_conv, first_conv_train, first_conv_train_float,
                        pointwise_conv)
from .variables import MOBILENET_LAYERS

OUTPUTS = {5: "c3", 11: "c4", 13: "c5"}             # mobilenet_v1.py:69-73


def mobilenet_variable_shapes(params):
    """The backbone's subset of variables.variable_shapes(params): MobilenetV1/*, Conv2d_0 and statistics included."""
    from .variables import variable_shapes
    if params.get("backbone") != "mobilenet":
        raise ValueError("mobilenet_variable_shapes: the config's backbone is %r" % (params.get("backbone"),))
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("MobilenetV1/")}


class TrainableBackbone(ReferenceVariables):
    """What the trainable backbones share: the first convolution, frozen by default or trained with the rest
    (train_first, 4.14), from uint8 or float32 frames (4.16).  A subclass states FIRST (the first convolution's scope), BN_LEAF (the
    batch-norm scope under every convolution), ACT (the first convolution's activation, and _bn's default) and the frame-size rule
    SIZE_MULTIPLE with SIZE_MESSAGE; it checks its config, hands its variable shapes over and keeps its graph.

    shapes   {reference variable name: shape} of the whole backbone; every one must be in `weights` (a missing one is a KeyError,
             not a draw).  Those under FIRST are kept as frozen arrays unless train_first; the others become the module's variables."""

    FIRST = BN_LEAF = ACT = SIZE_MULTIPLE = SIZE_MESSAGE = None

    def __init__(self, shapes, params, weights, device, seed, keep_features, train_first):
        self.train_first = bool(train_first)
        frozen = {}
        for name, shape in shapes.items():
            if name.startswith(self.FIRST + "/") and not self.train_first:
                a = weights.get(name)
                if a is None:
                    raise KeyError("weights has no variable %r" % name)
                a = np.ascontiguousarray(a, dtype=np.float32)
                if tuple(a.shape) != tuple(shape):
                    raise ValueError("variable %r has shape %s, expected %s" % (name, a.shape, tuple(shape)))
                frozen[name] = a.copy()
        trained = {k: v for k, v in shapes.items() if self.train_first or not k.startswith(self.FIRST + "/")}
        super().__init__(trained, weights, lambda name, shape, rng: None, device, seed)
        self._frozen = frozen
        self._frozen_dev = {}
        self.params = dict(params)
        self.keep_features = bool(keep_features)
        self.features = {}
        if self.train_first:
            return
        mean, variance, gamma, beta = (frozen["%s/%s/%s" % (self.FIRST, self.BN_LEAF, leaf)]
                                       for leaf in ("moving_mean", "moving_variance", "gamma", "beta"))
        sf = gamma * (np.float32(1.0) / np.sqrt(variance + np.float32(BATCH_NORM_EPSILON)))
        self._first_bn = (mean, sf.astype(np.float32), beta)

    def frozen_variables(self):
        """{reference name: float32 array} of the first convolution: its kernel, gamma, beta and moving statistics, untouched by
        training ({} with train_first)."""
        return {k: v.copy() for k, v in self._frozen.items()}

    def _frozen_on(self, device):
        """The first convolution's frozen arrays on `device` for the float route: plain tensors, no variables (no gradient, not in
        named_variables() / statistics()), copied once per device from the arrays frozen_variables() returns."""
        dev = self._frozen_dev.get(device)
        if dev is None:
            dev = self._frozen_dev[device] = {k: torch.from_numpy(v.copy()).to(device) for k, v in self._frozen.items()}
        return dev

    def _bn(self, x, scope, act=None):
        return self.batch_norm_relu([x], ["%s/%s" % (scope, self.BN_LEAF)], act=act or self.ACT)[0]

    def first_conv(self, images):
        """The first convolution: frames -> pixel values in [-1, 1] -> 3x3 stride 2 -> batch norm -> ACT, from uint8 frames
        (2u/255 - 1) or from float32 frames in [0, 1] (2x - 1: TrainPipeline's batches; on u * (1 / 255) the bits of the uint8
        route).  Frozen: the engine's inference form on the moving statistics -- uint8: ssd.first_conv; float32: the raw float
        convolution on a device copy of the frozen kernel, then the inference batch norm + ACT, without a gradient.  train_first:
        the raw convolution with a weight gradient, then the batch norm in the module's mode."""
        from . import ssd
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype in (torch.uint8, torch.float32) and images.dim() == 4
                and images.shape[3] == 3):
            raise TypeError("images must be a uint8 or float32 [B,H,W,3] tensor on a GPU")
        if images.shape[1] % self.SIZE_MULTIPLE or images.shape[2] % self.SIZE_MULTIPLE:
            raise ValueError(self.SIZE_MESSAGE)
        raw = first_conv_train_float if images.dtype == torch.float32 else first_conv_train
        if self.train_first:
            return self._bn(raw(images, self.variable(self.FIRST + "/weights")), self.FIRST)
        if images.dtype == torch.float32:
            f = self._frozen_on(images.device)
            with torch.no_grad():
                bn = [f["%s/%s/%s" % (self.FIRST, self.BN_LEAF, leaf)] for leaf in ("gamma", "beta", "moving_mean", "moving_variance")]
                return batch_norm_act(raw(images, f[self.FIRST + "/weights"]), *bn, training=False, act=self.ACT)
        with torch.cuda.device(images.device):
            return ssd.first_conv(images.contiguous(), self._frozen[self.FIRST + "/weights"], self._first_bn, self.ACT)


class TrainableMobileNet(TrainableBackbone):
    """mobilenet_v1(images, is_training, depth_multiplier) (mobilenet_v1.py:7-73) as a torch.nn.Module on the HIP kernels, with
    Conv2d_0 frozen by default.

    params   the model config (backbone "mobilenet", depth_multiplier <= 1.0: the batch norm takes at most 1024 channels)
    weights  {reference variable name: float32 array in TF layout}; every MobilenetV1/* variable must be there (the reference never
             initialises a backbone from scratch: a missing one is a KeyError, not a draw)
    forward(images uint8 or float32 [B,H,W,3] on the GPU, at the network's size: H and W even) -> [c3, c4, c5] NHWC float32, the outputs of
    Conv2d_5, Conv2d_11 and Conv2d_13's pointwise layers.  .train(): batch statistics through batch_norm_act, the moving statistics
    of Conv2d_1 .. 13 move; .eval(): the engine's c3, c4, c5 bit for bit (raw depthwise, the inference batch norm + ReLU6, the raw
    1x1, the inference batch norm + ReLU6).  named_variables() / statistics() hold Conv2d_1 .. 13 only; frozen_variables() returns
    the Conv2d_0 arrays for TrainStep(..., frozen=backbone.frozen_variables()).  keep_features=True keeps the 26 post-activation
    tensors of the last forward in .features under the reference's features[layer_name] names (detached).
    train_first=True trains Conv2d_0 too: its kernel, gamma and beta join named_variables() (81 variables) and its moving statistics
    statistics() (54), frozen_variables() returns {}; .train() runs first_conv_train and batch_norm_act on batch statistics (Conv2d_0's
    moving statistics move), .eval() the same raw convolution and the inference batch norm + ReLU6 -- still the engine's c3, c4, c5
    bit for bit; keep_features=True also keeps features["Conv2d_0"].
    float32 frames are the batches TrainPipeline yields, in [0, 1] (pixel value 2x - 1): first_conv_train_float in
    place of first_conv_train, the same batch norm; with Conv2d_0 frozen the raw float convolution on the frozen kernel and the
    inference batch norm + ReLU6.  On frames u * (1 / 255) every result has the bits of the uint8 frames u."""

    FIRST, BN_LEAF, ACT = "MobilenetV1/Conv2d_0", "BatchNorm", "relu6"
    SIZE_MULTIPLE, SIZE_MESSAGE = 2, "images: even height and width (the network's size)"

    def __init__(self, params, weights, device=None, seed=0, keep_features=False, train_first=False):
        if params.get("backbone") != "mobilenet":
            raise ValueError("TrainableMobileNet: the config's backbone is %r" % (params.get("backbone"),))
        if float(params["depth_multiplier"]) > 1.0:
            raise ValueError("TrainableMobileNet: depth_multiplier above 1.0 is not supported (the batch norm takes at most 1024 channels)")
        super().__init__(mobilenet_variable_shapes(params), params, weights, device, seed, keep_features, train_first)

    def body(self, x):
        """Conv2d_1 .. Conv2d_13 on Conv2d_0's output [B,H,W,C0] -> [c3, c4, c5]."""
        feats, outs = {}, []
        for i, (stride, _f) in enumerate(MOBILENET_LAYERS, 1):
            s = "MobilenetV1/Conv2d_%d_depthwise" % i
            x = self._bn(depthwise_conv(x, self.variable(s + "/depthwise_weights"), stride), s)
            feats["Conv2d_%d_depthwise" % i] = x
            s = "MobilenetV1/Conv2d_%d_pointwise" % i
            x = self._bn(pointwise_conv(x, self.variable(s + "/weights")), s)
            feats["Conv2d_%d_pointwise" % i] = x
            if i in OUTPUTS:
                outs.append(x)
        self.features = {k: v.detach() for k, v in feats.items()} if self.keep_features else {}
        return outs

    def forward(self, images):
        x = self.first_conv(images)
        outs = self.body(x)
        if self.keep_features and self.train_first:
            self.features["Conv2d_0"] = x.detach()
        return outs
