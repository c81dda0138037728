"""The trainable FPN: detector/feature_extractor.py's fpn() in TRAIN mode on this project's own kernels (include/ssd_hip.h, "the
TRAIN FPN").

    TrainPipeline -> Engine (frozen backbone, retained c3, c4, c5) -> TrainableFPN -> TrainableBoxPredictor -> differentiable_loss
                  -> backward (HIP) -> TrainStep over both modules' variables -> checkpoint -> Detector / evaluation

This is the reference's own recipe (train.py:44-50 warm-starts only the backbone; fpn/*, box_net/* and class_net/* start from
their initialisers and are trained).  On features that do not require a gradient (an Engine's: a frozen backbone) no gradient
flows into c3, c4, c5; on features that do (TrainableMobileNet's, backbone_train.py) the backward also returns
d c3, d c4, d c5.  The FPN's graph is ONE torch.autograd.Function over train_ops.py's allocating helpers around train_calls.py's conv_forward / conv_backward (ssd_conv_train_forward / _backward); its backward runs
the gradients in a fixed order with ssd_fpn_merge_backward doing every sum, so torch provides memory, streams and the autograd
graph only.  The ops (conv_same, batch_norm_relu, fpn_merge_backward) and the variable loading (ReferenceVariables) are
train_ops.py's; this file keeps the FPN's initialisers and its graph.
"""
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .train_ops import ReferenceVariables, _conv_backward, _conv_forward, _need, fpn_merge_backward

FPN_DEPTH = 256                 # detector/feature_extractor.py:7
LEVELS = (3, 4, 5, 6, 7)


class _FpnGraph(torch.autograd.Function):
    """fpn() before its batch norms (feature_extractor.py:57-69) as one node: (c3, c4, c5, the ten kernels) -> raw p3 .. p7.  The
    backward is the fixed sequence of DESIGN.md 4.12.  When none of c3, c4, c5 requires a gradient that is all of it; when one
    does, the three laterals' weight-gradient calls become ssd_pointwise_train_backward with the data gradient and p6's gives its
    stride-2 data gradient too: d c3 = lateral3^T(d x3), d c4 = lateral4^T(d x4), d c5 = lateral5^T(d x5) +
    dx_p6(d p6), the sum by ssd_fpn_merge_backward."""

    @staticmethod
    def forward(ctx, c3, c4, c5, l3, l4, l5, k3, k4, k5, k6, k7):
        c3, c4, c5 = c3.contiguous(), c4.contiguous(), c5.contiguous()
        ks = tuple(k.contiguous() for k in (l3, l4, l5, k3, k4, k5, k6, k7))
        l3, l4, l5, k3, k4, k5, k6, k7 = ks
        x5, = _conv_forward((c5,), l5, None, 1, None)
        p5, = _conv_forward((x5,), k5, None, 1, None)
        p6, = _conv_forward((c5,), k6, None, 2, None)
        r6 = fpn_merge_backward(p6, gate=p6, same_size=True)            # relu(p6): +0 + (p6 > 0 ? p6 : +0)
        p7, = _conv_forward((r6,), k7, None, 2, None)
        x4, = _conv_forward((c4,), l4, None, 1, (x5,))
        p4, = _conv_forward((x4,), k4, None, 1, None)
        x3, = _conv_forward((c3,), l3, None, 1, (x4,))
        p3, = _conv_forward((x3,), k3, None, 1, None)
        ctx.save_for_backward(c3, c4, c5, x3, x4, x5, p6, r6, *ks)
        ctx.shape7 = tuple(p7.shape)
        return p3, p4, p5, p6, p7

    @staticmethod
    @once_differentiable
    def backward(ctx, d3, d4, d5, d6, d7):
        c3, c4, c5, x3, x4, x5, p6, r6, l3, l4, l5, k3, k4, k5, k6, k7 = ctx.saved_tensors
        z = lambda d, like: torch.zeros_like(like) if d is None else d.contiguous()
        d3, d4, d5, d6 = z(d3, x3), z(d4, x4), z(d5, x5), z(d6, p6)
        d7 = torch.zeros(ctx.shape7, dtype=torch.float32, device=r6.device) if d7 is None else d7.contiguous()
        g7, _, (dr6,) = _conv_backward((r6,), k7, (d7,), 2, True)
        dp6 = fpn_merge_backward(dr6, base=d6, gate=p6, same_size=True)  # d p6 (raw) = d p6 from its batch norm + relu'(p6) * d relu(p6)
        bridge = any(ctx.needs_input_grad[:3])                           # a trainable backbone: also d c3, d c4, d c5

        def lateral(c, l, dx):
            gl, _, dcs = _conv_backward((c,), l, (dx,), 1, bridge, entry="pointwise" if bridge else "conv")
            return gl, dcs[0] if bridge else None
        g6, _, dc5_p6 = _conv_backward((c5,), k6, (dp6,), 2, bridge)
        g3, _, (dx3,) = _conv_backward((x3,), k3, (d3,), 1, True)
        gl3, dc3 = lateral(c3, l3, dx3)
        g4, _, (dx4,) = _conv_backward((x4,), k4, (d4,), 1, True)
        fpn_merge_backward(dx3, base=dx4, out=dx4)                      # d x4 = d x4 from p4 + the 2x2 sums of d x3
        gl4, dc4 = lateral(c4, l4, dx4)
        g5, _, (dx5,) = _conv_backward((x5,), k5, (d5,), 1, True)
        fpn_merge_backward(dx4, base=dx5, out=dx5)                      # d x5 = d x5 from p5 + the 2x2 sums of d x4
        gl5, dc5 = lateral(c5, l5, dx5)
        if bridge:
            fpn_merge_backward(dc5_p6[0], base=dc5, same_size=True, out=dc5)    # d c5 = lateral5^T(d x5) + dx_p6(d p6)
            dc3, dc4, dc5 = [d if need else None for d, need in zip((dc3, dc4, dc5), ctx.needs_input_grad[:3])]
        return dc3, dc4, dc5, gl3, gl4, gl5, g3, g4, g5, g6, g7


def fpn_variable_shapes(params):
    """The FPN's subset of variables.variable_shapes(params): fpn/*, statistics included."""
    from .variables import variable_shapes
    return {k: v for k, v in variable_shapes(params).items() if k.startswith("fpn/")}


def variance_scaling_draw(rng, shape):
    """tf.variance_scaling_initializer() with its defaults (scale 1, fan-in, truncated normal) for an HWIO kernel: every element
    is drawn from a normal distribution of standard deviation s = sqrt(1 / fan_in) / 0.87962566103423978, fan_in = k * k * Cin,
    and re-drawn while it lies outside [-2 s, 2 s]; the constant is the standard deviation of the unit normal truncated at +-2,
    so the kept values have variance 1 / fan_in.  `rng` is a numpy Generator; the draw order is C order, re-draws appended (this
    library's choice: TF's own random stream is not reproduced)."""
    fan_in = int(np.prod(shape[:-1]))
    s = math.sqrt(1.0 / fan_in) / 0.87962566103423978
    a = rng.normal(0.0, s, shape)
    bad = np.abs(a) > 2.0 * s
    while bad.any():
        a[bad] = rng.normal(0.0, s, int(bad.sum()))
        bad = np.abs(a) > 2.0 * s
    return a.astype(np.float32)


class TrainableFPN(ReferenceVariables):
    """fpn(features, is_training) (feature_extractor.py:40-76) as a torch.nn.Module on the HIP kernels.

    params   the model config (backbone, depth_multiplier: config.load_config)
    weights  {reference variable name: float32 array in TF layout}; only fpn/* is read.  A variable that is missing -- train.py's
             warm start, where `weights` holds the backbone only -- is drawn with the reference's initialiser: kernels by
             variance_scaling_draw(numpy default_rng(seed), shape) in variables.variable_shapes order, gamma 1, beta 0,
             moving_mean 0, moving_variance 1.
    forward([c3, c4, c5], NHWC, e.g. from ssd.BackboneFeatures) -> [p3, p4, p5, p6, p7]; p7 = conv(relu(RAW p6)), the batch norms
    come last (:71-74).  A feature that requires a gradient (TrainableMobileNet's outputs) receives one; a feature that does not (an
    Engine's: a frozen backbone) is detached, and with three such features the backward is the frozen-backbone sequence, launch for
    launch.  .train(): batch statistics, the moving statistics move; .eval(): the
    engine's inference form, bit for bit.  named_variables() / statistics() are what TrainStep takes, e.g. together with the head's:
    TrainStep({**fpn.named_variables(), **head.named_variables()}, config, {**fpn.statistics(), **head.statistics()}, layout="tf",
    params=params)."""

    def __init__(self, params, weights, device=None, seed=0):
        def initial(name, shape, rng):
            if weights.get(name) is not None:                           # present in another shape: an error, not a re-draw
                return None
            leaf = name.rsplit("/", 1)[1]
            return (variance_scaling_draw(rng, shape) if leaf == "kernel" else
                    np.ones(shape) if leaf in ("gamma", "moving_variance") else np.zeros(shape))
        super().__init__(fpn_variable_shapes(params), weights, initial, device, seed)
        self.params = dict(params)

    def forward(self, features):
        feats = list(features)
        if len(feats) != 3:
            raise ValueError("features: [c3, c4, c5]")
        for f in feats:
            _need(f, "features")
        kernels = [self.variable("fpn/lateral%d/kernel" % i) for i in (3, 4, 5)] + [self.variable("fpn/p%d/kernel" % i) for i in LEVELS]
        raw = _FpnGraph.apply(*[f if f.requires_grad else f.detach() for f in feats], *kernels)
        return self.batch_norm_relu(list(raw), ["fpn/p%d_batch_norm" % i for i in LEVELS])
