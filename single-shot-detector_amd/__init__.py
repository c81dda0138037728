"""MI355X-native RetinaNet inference path (drop-in for the reference's inference/detector.py
+ detector/ssd.py).  Import as `ssd_amd` (see ssd_amd.py at the repository root: the
directory name `single-shot-detector_amd` is not a Python identifier).

Host code is Python; all arithmetic runs in hand-written HIP kernels for gfx950 behind the
C ABI of include/ssd_hip.h (csrc/libssd_hip.so, loaded with ctypes).  PyTorch is used only
for device memory, streams and torch.distributed.  There is NO CPU fallback: every op
raises if the HIP library is missing or no GPU is present.
"""
from .config import load_config, INFERENCE_KEYS, load_loss_config, LOSS_KEYS, load_train_config, TRAIN_KEYS   # noqa: F401
from .config import load_optimizer_config, OPTIMIZER_KEYS, load_run_config, RUN_KEYS   # noqa: F401
from .variables import (variable_shapes, synthetic_weights, save_weights,   # noqa: F401
                        load_weights)
from .pb_import import read_frozen_graph, load_pb_weights             # noqa: F401
from .ckpt_import import (read_checkpoint, read_checkpoint_index, resolve_checkpoint,   # noqa: F401
                          load_ckpt_weights, crc32c)
from ._lib import build, lib, lib_path, SsdError, set_option, get_option                       # noqa: F401
from .ssd import (SSD, AnchorGenerator, RetinaNetFeatureExtractor, RetinaNetBoxPredictor, BackboneFeatures,     # noqa: F401
                  batch_multiclass_non_max_suppression, network_input_size, Engine,
                  get_training_targets, ssd_loss, ssd_loss_backward, differentiable_loss, level_top_means)
from .detector import Detector                                         # noqa: F401
from . import tiles                                                    # noqa: F401  (Detector.detect_tiled's grid, gather and merge)
from .tiles import tile_grid                                           # noqa: F401
from . import jpeg                                                     # noqa: F401  (JPEG bytes -> frames on the GPU)
from .jpeg import JpegDecoder, JpegEncoder                             # noqa: F401
from . import coco_eval, coco_metric, coco_match, coco_accumulate, coco_rows, voc_match, tfrecords            # noqa: F401  (evaluation: `python -m ssd_amd.evaluation`, imported on use)
from .distributed import shard_range, all_gather_detections, detect_sharded, bind_to_gpu_numa_node  # noqa: F401
from .distributed import (ChunkAssignment, detect_many_sharded, node_device_and_backend, init_node_process_group,  # noqa: F401
                          launch_local)
from .augment import augment_batch, sample_augmentation, TrainPipeline   # noqa: F401
from .train_step import TrainStep                                     # noqa: F401
from . import train_calls                                             # noqa: F401  (how the TRAIN entry points are called)
from .train_calls import histogram_limits                             # noqa: F401
from . import metric_calls                                            # noqa: F401  (what the metrics' GPU paths share round their entry points)
from . import summaries                                               # noqa: F401  (TensorBoard event files, by hand)
from .train_ops import (conv_same, conv3x3_same, batch_norm_relu, batch_norm_act, depthwise_conv, pointwise_conv,   # noqa: F401
                        fpn_merge_backward, first_conv_train, first_conv_train_float, concat_shuffle_split, concat_channels, maxpool3x3s2_train)
from .head_train import TrainableBoxPredictor, head_variable_shapes   # noqa: F401
from .fpn_train import TrainableFPN, fpn_variable_shapes, variance_scaling_draw   # noqa: F401
from .backbone_train import TrainableMobileNet, mobilenet_variable_shapes   # noqa: F401
from .shufflenet_train import TrainableShuffleNet, shufflenet_variable_shapes   # noqa: F401
from .grad_exchange import GradientExchange                           # noqa: F401  (data-parallel training's one collective)
from .trainer import Trainer                                        # noqa: F401  (`python -m ssd_amd.train`: train.py's loop)
