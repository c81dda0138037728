/*
 * ssd_hip.h -- C ABI of libssd_hip.so: the MI355X (gfx950) RetinaNet inference path
 * that replaces the TensorFlow session behind TropComplique/single-shot-detector's
 * `Detector` (reference paths below are relative to the reference repository).
 *
 * The reference has no FFI/plugin layer of its own (it is Python on TF 1.12); the
 * boundary it does have is the frozen graph's tensor contract
 *     images:0 uint8 [1,H,W,3]  ->  boxes:0 [1,2000,4] f32, labels:0 [1,2000] i32,
 *                                   scores:0 [1,2000] f32, num_boxes:0 [1] i32
 * (create_pb.py:40,72; inference/detector.py:21-27,51-52; model.py:70-73).  ssd_forward()
 * is that `sess.run`, generalised over the batch dimension.  The other entry points are
 * the pieces the graph is assembled from, exported so that each can be parity-tested
 * against the CPU oracle exactly where the reference defines it.
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is device (HIP) memory owned by the
 *     caller, every pointer named *_host is host memory; the library owns its weights
 *     and workspace arena.
 *   - layout NHWC fp32, conv kernels HWIO, exactly the reference's TF variable layout.
 *   - return value: 0 (SSD_OK) or a negative code; ssd_last_error() gives the text for
 *     the calling thread.  Nothing throws across the ABI.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  ssd_postprocess only
 *     enqueues work.  ssd_forward only enqueues work for a shape it has a layer plan for.  Plans
 *     are keyed on what the NETWORK sees -- batch, the resized + padded height and width -- and a
 *     handle KEEPS the plans of every shape it has served (the reference's graph takes any image
 *     size in one session, detector/ssd.py:27-31, create_pb.py:24,40; its accuracy harness feeds
 *     val2017's mix of sizes through one Detector, inference/evaluate_on_COCO.ipynb:125-150): the
 *     FIRST call that lands on a new network shape -- and the first after ssd_set_precision or a
 *     handle option change -- builds that shape's plan beside the others (allocates its arena,
 *     uploads the anchor table; no device-wide wait), later calls of any source size that resizes
 *     to it call no HIP API but kernel launches.  The plans' arenas are bounded by option
 *     "plan_cache_mb"; passing it evicts the least recently used plans, which drains the device
 *     (only then).  ssd_plan_cache_stats reports the cache.
 *     ssd_status, ssd_get_tensor and ssd_set_precision synchronise (documented at each).  The
 *     stage entry points that take host weights (ssd_conv2d, ssd_depthwise3x3, ssd_dw_pw,
 *     ssd_first_conv, ssd_concat_shuffle_split, ssd_shuffle_conv1x1) are test conveniences and synchronise before
 *     returning.
 *   - one handle per device.  Every entry point that takes a handle holds the handle's mutex, so concurrent calls on
 *     one handle are serialised by the library, and a forward enqueued on another stream than the previous one first
 *     waits for that one's last kernel (a shape's arena is one, and the plans share the library's internal streams): two host
 *     threads may share a handle the way they
 *     may share a tf.Session (inference/detector.py:34,52).  The OUTPUT buffers belong to the caller, who must not let
 *     two in-flight forwards write the same ones.
 */
#ifndef SSD_HIP_H
#define SSD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_OK 0
#define SSD_ERR_INVALID (-1)   /* bad argument / unsupported shape           */
#define SSD_ERR_HIP (-2)       /* a HIP runtime call failed                  */
#define SSD_ERR_STATE (-3)     /* call out of order (e.g. forward before finalize) */
#define SSD_ERR_WEIGHT (-4)    /* missing / mis-shaped / unknown variable    */
#define SSD_ERR_UNSUPPORTED (-5)   /* a well-formed JPEG of a kind the decoder does not take (block "the JPEG decoder") */

#define SSD_ACT_NONE 0
#define SSD_ACT_RELU 1         /* tf.nn.relu  */
#define SSD_ACT_RELU6 2        /* tf.nn.relu6 */

#define SSD_BACKBONE_MOBILENET 0   /* detector/backbones/mobilenet_v1.py  */
#define SSD_BACKBONE_SHUFFLENET 1  /* detector/backbones/shufflenet_v2.py */

/* Arithmetic of the dense convolutions (ssd_set_precision): FPN laterals and 3x3 outputs, head
 * towers, class / box heads, and the MobileNet pointwise layers that are not fused with their
 * depthwise convolution (Conv2d_5..13).  Depthwise layers, the first convolution, the fused
 * depthwise+pointwise blocks and the ShuffleNet backbone are exact fp32 in both modes.  The
 * reference graph is fp32 end to end (tf.float32 everywhere, model.py:13-77): F32 is the default
 * and the mode every parity statement and the benchmark's headline refer to; F16X3 is opt-in.
 *   F32    every product on the exact-fp32 matrix instruction, one k-ordered fmaf chain per
 *          output: bit-identical to the CPU oracle.
 *   F16X3  each fp32 operand is carried as two halves x = h + l (22 significand bits) and a
 *          product is evaluated as xh*wh + xh*wl + xl*wh on the fp16 matrix instruction with
 *          fp32 accumulation: the error of one convolution equals that of an fp32 accumulation
 *          chain (measured), but the summation ORDER differs from the oracle's, so
 *          results agree within the north-star tolerance (1e-4), not bit for bit. */
#define SSD_PRECISION_F32 0
#define SSD_PRECISION_F16X3 1

typedef struct ssd_handle ssd_handle;

/* The inference keys of config_mobilenet.json / config_shufflenet.json (:7-12,21),
 * consumed by model.py:22-30,46,57-61. */
typedef struct ssd_config {
    int32_t backbone;            /* SSD_BACKBONE_*                       */
    float depth_multiplier;      /* "depth_multiplier"                   */
    int32_t num_classes;         /* "num_classes"                        */
    float score_threshold;       /* "score_threshold"                    */
    float iou_threshold;         /* "iou_threshold"                      */
    int32_t max_boxes_per_class; /* "max_boxes_per_class"                */
    int32_t min_dimension;       /* "min_dimension" (create_pb.py:24)    */
    int32_t device;              /* HIP device index (visible_device_list, inference/detector.py:6) */
} ssd_config;

/* ---- lifetime: replaces Detector.__init__ (inference/detector.py:6-34) ------------- */
int ssd_create(const ssd_config *cfg, ssd_handle **out);
void ssd_destroy(ssd_handle *h);
const char *ssd_last_error(void);

/* Selects the arithmetic of the dense convolutions (list above) for the following ssd_forward
 * calls (synchronises and drops the cached layer plan when the mode changes).  A new handle
 * takes its mode from the environment variable SSD_PRECISION ("f32" | "f16x3"), default f32. */
int ssd_set_precision(ssd_handle *h, int32_t mode /* SSD_PRECISION_* */);
int ssd_get_precision(ssd_handle *h);
/* Options.  None changes a result bit in mode F32 (each selects among kernels or schedules that are bit-identical by
 * construction and by test); the library reads NO environment variable for them (SSD_PRECISION above is the only one it
 * reads).  `h` == NULL sets the process-wide value, which the handle-less stage entry points below use and which a handle
 * falls back to for an option it has not been given itself; with a handle the call synchronises and drops the cached layer
 * plan.  Keys (value; default).
 * Selectors a caller may want:
 *   "streams"         0 auto | 1: every kernel of a forward on the caller's stream, in plan order            (0)
 *   "h2d_chunks"      2 | 1..16: pieces of ssd_forward_host's staging copy + upload                           (2)
 *   "front_fuse"      -1 auto | 0 | 1: the backbone's first layers as one launch (front.hip): MobileNet's first
 *                     convolution + Conv2d_1, ShuffleNet's first convolution + max pool                       (-1)
 *   "fuse_dw"         -1 default | bit mask of depthwise+pointwise pairs that run as one launch (MobileNet: bit i =
 *                     Conv2d_{i+1}; ShuffleNet: non-zero = every unit)                                        (-1)
 *   "backbone_split"  0 auto | 1 .. 4 (ShuffleNet: 1 | 2): backbone chains (two half-batch chains on two streams from 4 images on) (0)
 *   "event_fence"     0 | 1: the library's stream-ordering events with the default flags (system-scope fence per record) (0)
 *   "plan_cache_mb"   0 auto (a quarter of the device's memory) | n: MiB of arena the handle's cached layer plans may hold;
 *                     the least recently used go first, the plan of the running shape always stays.  Setting it on a handle
 *                     evicts down to the new budget and does NOT drop the other plans                          (0)
 * Test hooks -- they pin a kernel variant or a plan shape so that the parity tests see every shape on it:
 *   "igemm_tile"      0 auto | 128 | 64 pin the tile of the 128x128-class launches | 20..27, 30 pin a tile of the latency form
 *                     wherever that form applies: 20..23 one wave per block (1x1, 1x2, 2x1, 2x2 sixteen-wide units), 24..27
 *                     two / four waves per block sharing the positions through LDS, 30 the one-wave tile with 16 K-steps of
 *                     operands in flight (the auto choice for the smallest launches).  Any other value is refused  (0)
 *   "igemm_lat"       1 | 0: small exact-fp32 launches on the latency form (v_mfma_f32_16x16x4_f32) | 2: ... and 1x1 launches
 *                     up to 1 280 tiles | 3: as 1 without fpn p6 / p7 of the serving batches                  (1)
 *   "igemm_deep64"    -1 auto | 0 | 1: 64x64 tiles with operand loads three K-steps ahead                     (-1)
 *   "igemm16"         -1 auto | 0 | 1: F16X3 launches on the 256x256-tile kernel                              (-1)
 *   "igemm_96"        1 | 0: 128x96 tiles for widths 96 divides and 128 does not (read by ssd_finalize)       (1)
 *   "lateral_split"   1 | 0: F16X3 laterals split fp32 rows while staging them                                (1)
 *   "fpn_group"       -1 auto | 0 | 1: fpn p3 + p4 + p5 as one grouped launch (batch <= 2, F32)               (-1)
 *   "fpn_p7_group"    1 | 0: fpn p7 as a fourth level of that launch                                          (1)
 *   "fpn_early_lat"   -1 auto | 0 | 1: lateral3 / lateral4 early, their top-down sums as one elementwise launch (batch <= 2) (-1)
 *   "nsub"            0 auto | 1..8: at least this many consecutive sub-batch plans (the split a batch whose tensors would
 *                     pass 2 GiB takes)                                                                        (0)
 *   "nms_fast_max"    -1 default | n >= 0: candidate lists up to n stay in one wave's registers               (-1)
 *   "first_conv_px"   1 | 0: the first convolution of RESIZED frames (any size that is not the network's own) on the
 *                     lane-per-pixel kernel / on the thread-per-4-channels kernel of rounds 1-5                (1)
 *   "debug_sync"      0 | 1: announce every op on stderr, run it alone, wait for it, print its time           (0)
 *   "logits_screen"   -1 auto | 0: the class logits as one dense launch | 1: screen + fill (an upper bound of every logit on the
 *                     f16 matrix pipe marks the octets the score filter cannot exclude, those are computed exactly; F32 only,
 *                     auto: from 32 768 rows on).  Detections are bit-identical; "class_predictions" is made whole by the dense
 *                     launch at its first read behind a screened forward (a caller that reads it every time sets 0) | 2: as 1
 *                     with the tensor pre-filled with 0xff bytes, for tests that read "class_logits_filled"     (-1)
 *   "hist_scheme"     -1 default | 0 .. 4: how ssd_train_histograms aggregates a wave's equal buckets before the LDS atomic
 *                     (its block below; process-wide only)                                                    (-1)
 * (Rounds 1-4 carried more switches -- schedule experiments that measured equal or slower: tower_group, head_serial,
 *  side_priority, level_split, fpn_p6_first, lat_one, dwpw_lat, graph, staggered sub-batch plans.  They are out of the library;
 *  scripts/experiments/README.md has what each measured and the commit that holds its source.)
 * ssd_get_option returns the value in effect (handle, else process), INT32_MIN when neither was set. */
int ssd_set_option(ssd_handle *h, const char *key, int32_t value);
int ssd_get_option(ssd_handle *h, const char *key, int32_t *value);
/* Synchronises the device and returns (and clears) the handle's status word.  Bit 0: in
 * F16X3 mode an activation left the fp16 range (|x| > 65504) and was clamped -- the results
 * of the forwards since the last call are not trustworthy; re-run them in F32 mode. */
int ssd_status(ssd_handle *h, int32_t *flags_out);

/* One call per TF variable of the frozen graph, by the reference's variable name
 * (e.g. "MobilenetV1/Conv2d_3_pointwise/weights", "fpn/p6/kernel",
 * "class_net/batch_norm_2_for_level_5/moving_variance"; SURVEY.md 8a "Weights").
 * Replaces tf.import_graph_def of the Const nodes (inference/detector.py:13-19). */
int ssd_load_weight(ssd_handle *h, const char *name, const float *host, const int64_t *shape,
                    int32_t ndim);
/* Checks that every variable of the configured architecture was loaded, computes the
 * batch-norm scale factors, re-lays the kernels out for the HIP kernels and uploads. */
int ssd_finalize(ssd_handle *h);

/* ---- the hot path: replaces sess.run(output_ops, {images: ...})
 *      (inference/detector.py:51-52) = create_pb.py:42-47 + model.py:13-77 ------------ */
/* images_dev uint8 [B,H,W,3], any H and W: the serving graph's preprocessing
 * (create_pb.py:42-47 -> resize_keeping_aspect_ratio(min_dimension, 128), pipeline.py:138-194:
 * nearest-neighbour resize so that the short side is min_dimension, zero pad bottom/right to
 * multiples of 128, box_scaler) is fused into the first kernel; for H, W multiples of 128 with
 * min(H,W) == min_dimension it is the identity.
 * Outputs, T = num_classes*max_boxes_per_class (2000): boxes_dev f32 [B,T,4]
 * (ymin,xmin,ymax,xmax, normalised, already divided by box_scaler, model.py:67-68),
 * labels_dev i32 [B,T], scores_dev f32 [B,T], num_boxes_dev i32 [B]; zero padded. */
int ssd_forward(ssd_handle *h, const uint8_t *images_dev, int32_t B, int32_t H, int32_t W,
                float *boxes_dev, int32_t *labels_dev, float *scores_dev,
                int32_t *num_boxes_dev, void *stream);

/* The same graph with the outputs as B fixed RECORDS -- the unit the all-gather of a data-parallel step moves (one process
 * per GPU, images sharded, detections exchanged once per batch; the reference maps over images, nms.py:96-101, and has no
 * multi-GPU code).  Record b starts at records_dev + b * ssd_record_words(h) 32-bit words:
 *     boxes [T,4] f32 | scores [T] f32 | labels [T] i32 | num_boxes i32      T = num_classes * max_boxes_per_class
 * (48 004 bytes at T = 2000).  records_dev: device memory, or pinned host memory (device-accessible at its own address).
 * Asynchronous on `stream` like ssd_forward. */
int32_t ssd_record_words(const ssd_handle *h);
int ssd_forward_records(ssd_handle *h, const uint8_t *images_dev, int32_t B, int32_t H, int32_t W,
                        void *records_dev, void *stream);
/* Detector.__call__'s own form (inference/detector.py:51-52 feeds a HOST array on every call): images_host is ordinary
 * (pageable) host memory; the library copies it through its pinned staging buffer into device memory in option
 * "h2d_chunks" pieces (piece k crosses the bus under the host copy of piece k + 1) and runs ssd_forward_records on
 * `stream`.  On return images_host may be reused; the upload and the forward are asynchronous on `stream`.
 * `records`: device memory or pinned host memory, as for ssd_forward_records. */
int ssd_forward_host(ssd_handle *h, const uint8_t *images_host, int32_t B, int32_t H, int32_t W,
                     void *records, void *stream);

/* Frames of DIFFERENT sizes as ONE batch.  The reference's graph is fed one image per call because a tensor has one height and
 * width (create_pb.py:40); what the network sees, though, is the size AFTER resize_keeping_aspect_ratio (pipeline.py:138-194), and
 * frames of many source sizes share it (480x640, 375x500, 333x500 -> 640x896).  ssd_forward_mixed runs B <= 64 such frames through the
 * ordinary batched plan of that network shape: the first kernel reads every frame through its own geometry (passed in its
 * arguments: nothing is uploaded), the pack kernel divides every image's boxes by its own box_scaler (model.py:67-68).  Record b
 * is bit for bit what frame b gives alone.
 *   images_dev   base pointer of the frames, uint8; frame b = [hw_host[2b], hw_host[2b+1], 3] at byte offset offsets_host[b]
 *                (offsets_host == NULL: back to back, every frame on the next 16-byte boundary); all within 2 GiB of the base
 *   records_dev  B records as for ssd_forward_records (device or pinned host memory)
 * Every frame must resize to the same network shape (ssd_network_shape tells a caller which: group by it), else SSD_ERR_INVALID.
 * Asynchronous on `stream`; hw_host / offsets_host may be reused on return. */
int ssd_network_shape(ssd_handle *h, int32_t height, int32_t width, int32_t *net_hw_out /* [2] */);
int ssd_forward_mixed(ssd_handle *h, const uint8_t *images_dev, int32_t B, const int32_t *hw_host, const int64_t *offsets_host,
                      void *records_dev, void *stream);
/* ... fed from host memory: frames_host[b] points to frame b (pageable memory is fine); staged through the handle's pinned buffer,
 * one upload per frame (frame b crosses the bus under the host copy of frame b + 1).  On return the frames may be reused. */
int ssd_forward_mixed_host(ssd_handle *h, const uint8_t *const *frames_host, int32_t B, const int32_t *hw_host, void *records,
                           void *stream);

/* inference/detector.py:33-58 (Detector.__call__) for ONE frame as one call: ssd_forward_host with B = 1, the wait for
 * `stream`, and the score filter `scores > score_threshold` over the frame's num_boxes rows (order kept) from the record
 * into the caller's host arrays boxes_out [capacity,4], labels_out / scores_out [capacity]; *n_out = rows kept.
 * `record` must be HOST-VISIBLE device-accessible memory of ssd_record_words(h) words (pinned: hipHostMalloc / a pinned
 * torch tensor): the last kernel writes the frame's record there and this call reads it.  A pointer that is not pinned or
 * managed host memory (device memory, pageable memory) is refused with SSD_ERR_INVALID -- checked once per pointer. */
int ssd_detect_host(ssd_handle *h, const uint8_t *image_host, int32_t H, int32_t W, float score_threshold,
                    void *record, float *boxes_out, int32_t *labels_out, float *scores_out, int32_t capacity,
                    int32_t *n_out, void *stream);

/* Copy a retained intermediate of the last ssd_forward to the host in the reference's
 * logical NHWC channel order (synchronises).  Names: "c3","c4","c5" (backbone outputs),
 * "p3".."p7" (feature_extractor.py:71-76), "encoded_boxes" [B,N,4] and
 * "class_predictions" [B,N,C] (box_predictor.py:102-104).  dims_out receives 4 ints. */
int ssd_get_tensor(ssd_handle *h, const char *name, float *host_dst, int64_t capacity_floats,
                   int32_t *dims_out);

/* Same, device to device: dst_dev receives the tensor in logical channel order; enqueued
 * on `stream` without synchronising (SSD.raw_predictions, ssd.py:37-40). */
int ssd_get_tensor_dev(ssd_handle *h, const char *name, float *dst_dev, int64_t capacity_floats,
                       int32_t *dims_out, void *stream);

/* The handle's cache of layer plans (conventions at the top of this file).  out[0..7] = cached plan sets, bytes of arena they
 * hold, the budget in bytes (option "plan_cache_mb"), hits, misses, evictions since ssd_create, and the network shape (height,
 * width) the last forward ran at.  A hit = a forward that found its shape's plan; a miss = one that built it. */
int ssd_plan_cache_stats(ssd_handle *h, int64_t *out8);
/* Drains the device and drops every cached plan (the next forward of each shape rebuilds it); also forgets the record
 * pointers ssd_detect_host has verified. */
int ssd_plan_cache_clear(ssd_handle *h);

/* Per-kernel-class timing with HIP events on the forward's stream (bench.py roofline).
 * classes: 0 conv3x3 MFMA, 1 pointwise MFMA, 2 depthwise, 3 first conv, 4 postprocess,
 * 5 other, 6 fused depthwise+pointwise, 7 conv3x3 on the 256x256-tile f16x3 kernel (igemm16.hip;
 * class 0 then holds the remaining 3x3 launches).  total_ms of a class is the union of its kernels' intervals (the two head towers
 * overlap on two streams).  ssd_profile_read synchronises the recorded events. */
int ssd_profile_enable(ssd_handle *h, int32_t on);
int ssd_profile_read(ssd_handle *h, int32_t cls, double *total_ms, int64_t *launches,
                     double *flops, double *bytes);
int ssd_profile_reset(ssd_handle *h);

/* ---- pieces of the graph, each where the reference defines it ---------------------- */

/* AnchorGenerator.__call__ (anchor_generator.py:40-120) with model.py:37-42 constants. */
int32_t ssd_num_anchors(int32_t H, int32_t W);
int ssd_anchors(int32_t H, int32_t W, float *anchors_host /* [N,4] */);
/* AnchorGenerator(strides, scales, scale_multipliers, aspect_ratios).__call__ (anchor_generator.py:13-120) for any
 * hyper-parameters: n_levels strides / scales, anchors per location = n_mult * n_ratios in itertools.product order.
 * Returns the number of anchors N (>= 0) or a negative SSD_ERR_*; writes [N,4] when anchors_host != NULL and
 * capacity_rows >= N (call once with NULL to size the buffer). */
int64_t ssd_anchors_ex(int32_t H, int32_t W, int32_t n_levels, const int32_t *strides, const double *scales,
                       int32_t n_mult, const double *multipliers, int32_t n_ratios, const double *ratios,
                       float *anchors_host, int64_t capacity_rows);

/* Dense k x k convolution (k = 1 or 3) on the MFMA implicit-GEMM kernel:
 * slim.conv2d / tf.layers.conv2d / conv2d_same (mobilenet_v1.py:49,66;
 * layer_utils.py:15-43; box_predictor.py:117-130,144-154; feature_extractor.py:57-69).
 * out = act( bn( conv(in) ) + bias + upsample2(up) ), each term optional (NULL).
 * pad_beg: 1 for 'same' stride 1 and for conv2d_same stride 2 (explicit pad),
 * 0 for TF 'SAME' stride 2 on even sizes and for k = 1.
 * bn_*: moving_mean, gamma*rsqrt(var+eps), beta (batch_norm_relu, layer_utils.py:5-12).
 * up_dev: coarser map [B,OH/2,OW/2,Cout] added after nearest x2 upsampling
 * (feature_extractor.py:67,79-100).  Cin must be a multiple of 8.  Batch norm, bias and
 * up_dev are mutually exclusive (the reference's graph has no layer combining them). */
int ssd_conv2d(const float *in_dev, int32_t B, int32_t H, int32_t W, int32_t Cin,
               const float *w_host /* [k,k,Cin,Cout] */, int32_t k, int32_t Cout,
               int32_t stride, int32_t pad_beg, int32_t OH, int32_t OW,
               const float *bn_mean_host, const float *bn_sf_host, const float *bn_beta_host,
               const float *bias_host, const float *up_dev, int32_t act, float *out_dev,
               void *stream);

/* The same convolution in F16X3 arithmetic (see SSD_PRECISION_F16X3): fp32 tensors in and
 * out, the split-fp16 rows exist only inside the call.  Test entry point for the kernel the
 * F16X3 forward runs. */
int ssd_conv2d_f16x3(const float *in_dev, int32_t B, int32_t H, int32_t W, int32_t Cin,
                     const float *w_host /* [k,k,Cin,Cout] */, int32_t k, int32_t Cout,
                     int32_t stride, int32_t pad_beg, int32_t OH, int32_t OW,
                     const float *bn_mean_host, const float *bn_sf_host, const float *bn_beta_host,
                     const float *bias_host, const float *up_dev, int32_t act, float *out_dev,
                     void *stream);

/* depthwise_conv (depthwise_conv.py:5-26): 3x3, weights [3,3,C,1], optional BN + act. */
int ssd_depthwise3x3(const float *in_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                     const float *w_host, int32_t stride, int32_t pad_beg, int32_t OH,
                     int32_t OW, const float *bn_mean_host, const float *bn_sf_host,
                     const float *bn_beta_host, int32_t act, float *out_dev, void *stream);

/* depthwise_conv + BN + act followed by the 1x1 conv + BN + act that consumes it, as ONE kernel
 * (the MobileNet block, mobilenet_v1.py:59-67; shufflenet_v2.py:118-137 depthwise -> conv1x1_after):
 * the depthwise result stays in LDS (input patches staged by LDS-DMA, channels streamed in slices of
 * 32: any C, any H x W).  'SAME' padding; stride 2 needs even H, W; every tensor below 2 GiB
 * (SSD_ERR_INVALID otherwise). */
int ssd_dw_pw(const float *in_dev, int32_t B, int32_t H, int32_t W, int32_t C,
              const float *dw_w_host /* [3,3,C,1] */, int32_t stride, const float *dw_mean_host,
              const float *dw_sf_host, const float *dw_beta_host, int32_t dw_act,
              const float *pw_w_host /* [1,1,C,Cout] */, int32_t Cout, const float *pw_mean_host,
              const float *pw_sf_host, const float *pw_beta_host, int32_t pw_act,
              float *out_dev, void *stream);

/* uint8 image -> /255 -> 2x-1 -> 3x3 stride-2 'SAME' conv -> BN -> act, fused
 * (create_pb.py:42-47; mobilenet_v1.py:34,49; shufflenet_v2.py:37,50). */
int ssd_first_conv(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W,
                   const float *w_host /* [3,3,3,Cout] */, int32_t Cout,
                   const float *bn_mean_host, const float *bn_sf_host,
                   const float *bn_beta_host, int32_t act, float *out_dev, void *stream);

/* MobileNet's first three layers as ONE launch -- what the layer plan runs for frames that arrive at the network's input
 * size (option "front_fuse"): ssd_first_conv (create_pb.py:42-47; mobilenet_v1.py:34,49: 3 -> 32) followed by ssd_dw_pw at
 * stride 1 (mobilenet_v1.py:59-67: depthwise 3x3, pointwise 32 -> 64), the 32-channel tensor kept in LDS.  Only these
 * widths (C0 == 32, Cout == 64; SSD_ERR_INVALID otherwise); bit-identical to the two calls it replaces.
 * images_dev [B,H,W,3] uint8, H and W even; out_dev [B,H/2,W/2,Cout]. */
int ssd_front_block(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W,
                    const float *w0_host /* [3,3,3,C0] */, int32_t C0, const float *bn0_mean_host,
                    const float *bn0_sf_host, const float *bn0_beta_host, int32_t act0,
                    const float *dw_w_host /* [3,3,C0,1] */, const float *dw_mean_host,
                    const float *dw_sf_host, const float *dw_beta_host, int32_t dw_act,
                    const float *pw_w_host /* [1,1,C0,Cout] */, int32_t Cout, const float *pw_mean_host,
                    const float *pw_sf_host, const float *pw_beta_host, int32_t pw_act,
                    float *out_dev, void *stream);

/* ShuffleNet's first two layers as ONE launch -- what the layer plan runs for frames that arrive at the network's input size
 * (option "front_fuse"): ssd_first_conv (shufflenet_v2.py:37,50: 3 -> 24) followed by ssd_maxpool3x3s2 (:51-54), the
 * half-resolution tensor kept in LDS.  Only Cout == 24, H and W multiples of 4 (SSD_ERR_INVALID otherwise); bit-identical
 * to the two calls it replaces.  out_dev [B,H/4,W/4,Cout]. */
int ssd_first_conv_maxpool(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W,
                           const float *w_host /* [3,3,3,Cout] */, int32_t Cout,
                           const float *bn_mean_host, const float *bn_sf_host,
                           const float *bn_beta_host, int32_t act, float *out_dev, void *stream);

/* slim.max_pool2d 3x3 stride 2 'SAME' (shufflenet_v2.py:51-54). */
int ssd_maxpool3x3s2(const float *in_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                     float *out_dev, void *stream);

/* concat_shuffle_split (shufflenet_v2.py:94-115) on [rows, D] tensors. */
int ssd_concat_shuffle_split(const float *x_dev, const float *y_dev, int64_t rows, int32_t D,
                             float *xo_dev, float *yo_dev, void *stream);

/* concat_shuffle_split (shufflenet_v2.py:94-115) followed by the unit's conv1x1_before + batch norm + activation (:119) on the
 * new x half, as the ONE kernel the layer plan runs for it (sn_pw.hip): the shuffle is the kernel's per-channel source table.
 * x_dev, y_dev [rows, D] (D even), w_host [1,1,D,Cout] -> out_dev [rows, Cout]; bit-identical to ssd_concat_shuffle_split
 * followed by ssd_conv2d on its first output. */
int ssd_shuffle_conv1x1(const float *x_dev, const float *y_dev, int64_t rows, int32_t D,
                        const float *w_host, int32_t Cout, const float *bn_mean_host, const float *bn_sf_host,
                        const float *bn_beta_host, int32_t act, float *out_dev, void *stream);

/* SSD.get_predictions (ssd.py:42-69) = sigmoid + batch_multiclass_non_max_suppression
 * (nms.py:48-102, decode box_utils.py:114-142, tf.image.non_max_suppression of TF r1.12)
 * + boxes /= box_scaler (model.py:67-68).
 * logits_dev [B,N,C], codes_dev [B,N,4], anchors_dev [N,4]; outputs as ssd_forward.
 * workspace_dev: ssd_postprocess_workspace_bytes(B,N,C,max_boxes_per_class) bytes. */
size_t ssd_postprocess_workspace_bytes(int32_t B, int32_t N, int32_t C,
                                       int32_t max_boxes_per_class);
int ssd_postprocess(const float *logits_dev, const float *codes_dev, const float *anchors_dev,
                    int32_t B, int32_t N, int32_t C, float score_threshold, float iou_threshold,
                    int32_t max_boxes_per_class, const float *box_scaler_host /* [4] or NULL */,
                    float *boxes_dev, int32_t *labels_dev, float *scores_dev,
                    int32_t *num_boxes_dev, void *workspace_dev, size_t workspace_bytes,
                    void *stream);

/* ---- the EVAL loss: model.py:79-104 in mode EVAL (train.py:61-65), without the regularisation term (host side) ----
 *
 * Matching (training_target_creation.py:48-130), targets (:133-176, box_utils.py:80-113) and the focal / smooth-L1 losses
 * (losses.py, ssd.py:71-133) on the GPU.  Every TF op is one fp32 op (no contraction); exp / log / log1p / sigmoid / pow
 * are correctly rounded (evaluated in double, rounded once); a reduce_sum is evaluated in double and rounded once, in a
 * fixed order: two calls give the same bits.
 *
 * Tie rule (single-sourced here, like the NMS order): TF's GPU argmax pins no tie order, this library takes the FIRST
 * index on ties -- per anchor the smallest gt index among those of maximal IoU, per gt the smallest anchor index among
 * those of maximal IoU (a gt whose IoUs are all 0 picks anchor 0).  The forced match of an anchor is the smallest gt that
 * picked it, whether or not that gt passes `iou >= 0.1`; it applies when ANY gt that picked it passes, and it overrides
 * whatever the anchor matched before (the collision of :69 is reproduced, not repaired).  An image with no gt: every
 * anchor -1.
 *
 * Arguments common to both entry points, all device memory of the caller:
 *   anchors_dev [N,4]     the UNCLIPPED anchors (AnchorGenerator, anchor_generator.py:116-117)
 *   gt_boxes_dev [B,G,4]  ymin,xmin,ymax,xmax in the frame of the anchors (box_scaler applied, pipeline.py:103-109)
 *   gt_labels_dev [B,G]   int32 in [0, C); gt_num_dev [B] int32: rows of image b used (clamped to [0, G]); with G == 0
 *                         gt_boxes_dev and gt_labels_dev are not read and may be NULL (every anchor -1)
 *   anchors_dev, gt_boxes_dev, codes_dev and reg_targets_dev 16-byte aligned (SSD_ERR_INVALID otherwise); G <= 4096.
 * Stream ordering the caller owes: both calls only ENQUEUE work on `stream`.  Tensors copied out of a handle
 * (ssd_get_tensor_dev) are ordered by that copy's stream.  A caller that points logits_dev / codes_dev straight at a
 * handle's retained tensors must enqueue on the stream of the NEXT forward of that handle, which starts behind it
 * (plan.hip enqueue_forward): on another stream the next forward may overwrite the arena while the loss reads it. */
#define SSD_LOSS_MAX_GT 4096
#define SSD_LOSS_MAX_LEVELS 8
typedef struct ssd_loss_config {
    double alpha;                  /* "alpha" (losses.py:39-43: alpha * x in fp32(alpha), (1 - alpha) formed in double) */
    float gamma;                   /* "gamma": tf.pow(1 - p_t, gamma)                                                    */
    float positives_threshold;     /* POSITIVES_THRESHOLD = 0.5 (constants.py:25)                                        */
    float negatives_threshold;     /* NEGATIVES_THRESHOLD = 0.5 (constants.py:26); < positives: -2 (ignore) in between   */
    int32_t n_levels;              /* 0 .. SSD_LOSS_MAX_LEVELS: entries of anchors_per_level (sum == N when > 0)          */
    int64_t anchors_per_level[SSD_LOSS_MAX_LEVELS];    /* num_anchors_per_feature_map (ssd.py:31-35)                    */
} ssd_loss_config;

size_t ssd_loss_workspace_bytes(int32_t B, int32_t N, int32_t G);
/* SSD._create_targets (ssd.py:165-199) = get_training_targets per image: reg_targets_dev f32 [B,N,4] (ty,tx,th,tw),
 * cls_targets_dev i32 [B,N] (label + 1, 0 = background), matches_dev i32 [B,N] (gt index, -1 negative, -2 ignore).
 * Each output may be NULL.  cfg: the thresholds (gamma, alpha and the levels are not read). */
int ssd_training_targets(const float *anchors_dev, int32_t N, const float *gt_boxes_dev, const int32_t *gt_labels_dev,
                         const int32_t *gt_num_dev, int32_t B, int32_t G, const ssd_loss_config *cfg,
                         float *reg_targets_dev, int32_t *cls_targets_dev, int32_t *matches_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
/* SSD.loss (ssd.py:71-133) on logits_dev [B,N,C] and codes_dev [B,N,4] (raw_predictions).
 *   per_image_dev f32 [B, 3 + n_levels]: localization sum, classification sum, matches, matches per level
 *                 (the image's own normaliser is max(matches, 1): EVAL runs at batch 1, pipeline.py:22-27)
 *   losses_dev f32 [2]: localization_loss, classification_loss, each / max(matches over the batch, 1) (ssd.py:120-133)
 *   cls_losses_dev, loc_losses_dev f32 [B,N] or NULL: the per-anchor losses (focal_loss / localization_loss outputs)
 * per_image_dev and losses_dev may be NULL too. */
int ssd_loss(const float *logits_dev, const float *codes_dev, const float *anchors_dev, int32_t B, int32_t N, int32_t C,
             const float *gt_boxes_dev, const int32_t *gt_labels_dev, const int32_t *gt_num_dev, int32_t G,
             const ssd_loss_config *cfg, float *per_image_dev, float *losses_dev, float *cls_losses_dev,
             float *loc_losses_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* The gradient of ssd_loss's losses_dev = (localization_loss, classification_loss) with respect to logits_dev [B,N,C] and
 * codes_dev [B,N,4], given the targets of ssd_training_targets (reg_targets_dev [B,N,4], cls_targets_dev [B,N],
 * matches_dev [B,N]) and ssd_loss's per_image_dev (row stride per_image_stride = 3 + n_levels floats; only column 2, the
 * matches, is read).  norm = max(sum over b of per_image[b][2], 1), the fp32 value ssd_loss divides by, is a constant
 * (as in TF: it depends only on the matching).  g = grad_losses_dev[0..1] (device f32 [2], the upstream gradients of
 * the two losses) or (1, 1) when NULL.  cfg supplies gamma and alpha only.
 *   d_logits_dev [b,a,c] = 0 when matches[b,a] == -2 (ignored), otherwise, with x the logit, z = 1 for the target class
 *     cls_targets - 1 (0 everywhere on background anchors), s = sigmoid(x), q = 1 - p_t = (z ? 1 - s : s),
 *     alpha_z = (z ? alpha : 1 - alpha) as ssd_loss forms them, nlp = max(x,0) - x*z + log1p(exp(-|x|)):
 *       alpha_z * (gamma * q^(gamma-1) * dq/dx * nlp + q^gamma * (s - z)) * g[1] / norm,  dq/dx = (z ? -1 : 1) * s(1-s);
 *     the first term is evaluated as gamma * q^gamma * (z ? -s : 1 - s) * nlp (dq/dx = +-q(1-q) folded in), which is 0
 *     where q == 0 -- its limit for every gamma > 0 -- and finite where q is denormal, gamma < 1 included.
 *   d_codes_dev [b,a,k] = 0 when matches[b,a] < 0, otherwise, with diff = codes - reg_targets (one fp32 op as in
 *     ssd_loss): (|diff| < 1 ? diff : sign(diff)) * g[0] / norm -- sign(diff) at |diff| == 1 (tf.where / tf.less).
 * Precision: each element is evaluated in double from its fp32 inputs (s and 1 - s both formed from exp(-|x|) without
 * cancellation) and rounded to fp32 once.  This is the exact derivative, not TF's autodiff chain op by op (parity with
 * TF's gradient is unpinned, like the forward's).  No atomics: two calls give the same bits.  Every output element is
 * written, zeros included: the caller need not clear d_logits_dev / d_codes_dev.  Enqueues only, on `stream`, under the
 * stream ordering of ssd_loss above.  NULL pointers, B, N or C < 1, C > 4194304, per_image_stride < 3, codes_dev /
 * reg_targets_dev / d_codes_dev not 16-byte aligned or any other pointer not 4-byte aligned: SSD_ERR_INVALID before any
 * HIP call. */
int ssd_loss_backward(const float *logits_dev, const float *codes_dev, int32_t B, int32_t N, int32_t C,
                      const float *reg_targets_dev, const int32_t *cls_targets_dev, const int32_t *matches_dev,
                      const float *per_image_dev, int32_t per_image_stride, const ssd_loss_config *cfg,
                      const float *grad_losses_dev, float *d_logits_dev, float *d_codes_dev, void *stream);

/* ---- the per-level top losses: the input of the `*_losses_on_level_*` histograms (ssd.py:135-152) ----
 *
 * Of every image and every pyramid level the top 20 % of the per-anchor losses, and their mean over the batch, slot by slot.  The
 * reference takes tf.nn.top_k(sorted=False), whose slot order TensorFlow leaves open; the SET it returns is defined, and at batch 1
 * the histogram of the mean is the histogram of that set.  For larger batches this library states its own order, single-sourced
 * here and unpinned against TF like the NMS and argmax tie rules: DESCENDING, so that slot j is the mean over the batch of each
 * image's j-th largest loss.
 * Inputs: plane 0 = cls_losses_dev, plane 1 = loc_losses_dev, ssd_loss's per-anchor outputs, float32 [B, N] with row stride N,
 *   4-byte aligned.  Levels: anchors_per_level[0 .. n_levels), 1 <= n_levels <= SSD_LOSS_MAX_LEVELS, every n_l >= 1, their sum == N;
 *   level l of image b is the slice [off_l, off_l + n_l) of row b, off_l the sum of the levels before it.
 * Count: k_l = ceil(n_l / 5).  The reference's ceil(fp32(n_l) * fp32(0.20)) (ssd.py:145) equals it for every n_l < 2^24 (the fp32
 *   product of a multiple of 5 never rounds past its integer); N >= 2^24 is refused.  ssd_loss_top_counts fills k_out[n_levels] and
 *   returns K = the sum of the k_l, or -1 for levels a call would refuse: the ONE definition of the count rule.
 * Order: the total order on bit patterns, key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) compared as uint32: -0.0 lies below
 *   +0.0, a NaN with the sign bit clear above +inf, a NaN with the sign bit set below -inf.  V[p][b][l][j], j = 0 .. k_l - 1, is the
 *   value whose key is the j-th largest of the segment.  Equal keys are equal values: ties need no rule.
 * Mean: M[p][l][j] = fp32( fp32( sum over b of (double)V[p][b][l][j] ) / fp32(B) ): the double sum runs from +0.0 in ascending b and
 *   is rounded once (the reduce_sum convention of the EVAL loss), then one correctly rounded fp32 division.  Non-finite values
 *   propagate (V holds their bits as they are; WHICH quiet NaN a mean over a NaN holds is not pinned).
 * Output: means_dev float32 [2][K], plane-major, level l at offset sum of k_l' over l' < l; every element is written.
 * Workspace: V, 2 * B * K floats, 16-byte aligned: ssd_loss_top_workspace_bytes (0 for a call that would be refused); its contents
 *   need no initialisation.
 * SSD_LOSS_TOP_MAX_K: the largest k_l a call takes (the sort buffer of one workgroup: 128 KiB of the 160 KiB of LDS), so n_l up to
 *   163840 -- level 3 of a 1280 x 1280 frame.
 * The call only enqueues two kernels on `stream`: no allocation, no host synchronisation, no floating-point atomics (integer LDS
 * atomics count keys; they change no bit): two calls give the same bytes.  Needs no handle.  SSD_ERR_INVALID before any HIP call: a
 * NULL plane or means_dev or one not 4-byte aligned; B < 1; n_levels outside [1, SSD_LOSS_MAX_LEVELS]; a NULL anchors_per_level; an
 * n_l < 1; N (or the levels' sum) >= 2^24; a k_l above SSD_LOSS_TOP_MAX_K; levels that do not sum to N; a NULL workspace, one not
 * 16-byte aligned or one smaller than the planner's figure. */
#define SSD_LOSS_TOP_MAX_K 32768
int64_t ssd_loss_top_counts(const int64_t *anchors_per_level, int32_t n_levels, int64_t *k_out);
size_t ssd_loss_top_workspace_bytes(int32_t B, const int64_t *anchors_per_level, int32_t n_levels);
int ssd_loss_top_means(const float *cls_losses_dev, const float *loc_losses_dev, int32_t B, int32_t N, const int64_t *anchors_per_level,
                       int32_t n_levels, float *means_dev, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the TRAIN input pipeline: Pipeline.augmentation after the decode (pipeline.py:117-135) ----
 *
 * The host decodes each JPEG and draws the image's random scalars (the crop window included: its rejection sampling reads the
 * boxes) and does all box arithmetic; this call does every per-pixel step of a batch in ONE launch, on uint8 frames, and
 * writes the float32 batch.  Per output element (y, x, c) of image b, with p = params[b]:
 *   1. source pixel    sy = p.crop_y + min(floor(y * (crop_h / out_h)), crop_h - 1), sx likewise with crop_x, crop_w, out_w: the
 *                      project's nearest-neighbour rule (the expression of first_pixels.h fc_src: floorf((float)dst * ((float)in /
 *                      (float)out)), the division correctly rounded), applied within the crop window
 *   2. convert         v = u8 * (float)(1.0 / 255.0)                                     (convert_image_dtype)
 *   3. colour          if SSD_AUG_COLOR: v = clip(v + color_offset[c], 0, 1)             (other_augmentations.py:16-28)
 *   4. grayscale       if SSD_AUG_GRAY: g = (R * 0.2989f + G * 0.5870f) + B * 0.1140f to all three channels (rgb_to_grayscale's
 *                      weights; the summation order is this library's choice)
 *   5. pixel scale     if SSD_AUG_SCALE: Philox4x32-10 with key philox_key (word 0 = the low 32 bits) on the counter
 *                      (y * out_w + x, 0, 0, 0), (y, x) the output position BEFORE the flip; word c for channel c becomes
 *                      u = as_float(0x3f800000 | (w & 0x7fffff)) - 1 (TF's Uint32ToFloat), then
 *                      v = clip(v * (u * scale_range + scale_min), 0, 1)                 (other_augmentations.py:101-106)
 *   6. flip            if SSD_AUG_FLIP: the element is stored to column out_w - 1 - x    (tf.image.flip_left_right)
 * Every step is one fp32 op at a time, without contraction (a numpy restatement is bit-exact); clip = min(max(v, 0), 1).  These
 * choices are single-sourced here and unpinned against TF.  An image's output depends on its own
 * parameters and frame only: not on its position in the batch, on B, or on the stream.
 *   images_dev   base pointer of the frames: frame b is uint8 [height, width, 3] (HWC, RGB) at byte offset params[b].offset; any
 *                size, any byte offset (bytes are gathered as bytes)
 *   params_host  the B parameter rows, read by this call to refuse bad ones; params_dev: the same rows in device memory (8-byte
 *                aligned), which the kernel reads -- the caller's upload, ordered before this call on `stream`
 *   out_dev      float32 [B, out_h, out_w, 3], or [B, 3, out_h, out_w] when channels_first != 0 (DATA_FORMAT); 16-byte aligned;
 *                every element is written
 * out_h and out_w: positive multiples of 128 (pipeline.py:32-33), out_h * out_w < 2^31.  Null pointers, B < 1, other sizes, a frame
 * with height or width < 1 or a negative offset, an empty crop window or one that leaves the frame, unknown flags:
 * SSD_ERR_INVALID before any HIP call.  Needs no handle; asynchronous on `stream`. */
#define SSD_AUG_COLOR 1
#define SSD_AUG_GRAY 2
#define SSD_AUG_SCALE 4
#define SSD_AUG_FLIP 8
typedef struct ssd_augment_params {          /* 64 bytes, no padding */
    int64_t offset;                          /* byte offset of the frame from images_dev                      */
    int32_t height, width;                   /* the frame                                                     */
    int32_t crop_y, crop_x, crop_h, crop_w;  /* the crop window in the frame's pixels                         */
    int32_t flags;                           /* SSD_AUG_* bits                                                */
    float color_offset[3];                   /* R, G, B offsets (SSD_AUG_COLOR)                               */
    float scale_min, scale_range;            /* minval, maxval - minval of random_pixel_value_scale (SSD_AUG_SCALE) */
    uint64_t philox_key;                     /* the image's Philox key (SSD_AUG_SCALE)                        */
} ssd_augment_params;
int ssd_augment(const uint8_t *images_dev, const ssd_augment_params *params_host, const ssd_augment_params *params_dev, int32_t B,
                int32_t out_h, int32_t out_w, int32_t channels_first, float *out_dev, void *stream);

/* ---- the TRAIN update: train_op after the gradients (model.py:106-128) ----
 *
 * Cosine-decayed Adam on every trainable variable, the weight-decay term's gradient folded into it, and the exponential moving
 * average (EMA) of every trainable variable, for a whole model in ONE launch.  TensorFlow's sources are not available to this
 * project: the formulas restate TF 1.12's ApplyAdam kernel, tf.train.cosine_decay and ExponentialMovingAverage.apply from memory.
 * What is pinned is the arithmetic below for given inputs, single-sourced here, NOT parity with TensorFlow.
 *
 * Let t = 1, 2, ... be the number of this update (global_step is t - 1 before it and t after it).  The host forms, in float64,
 * each rounded once to float32:
 *   lr    = initial_learning_rate * 0.5 * (1 + cos(pi * min(t - 1, num_steps) / num_steps))          (model.py:108-113)
 *   alpha = lr * sqrt(1 - 0.999^t) / (1 - 0.9^t),  lr the float32 value above                         (Adam's step size)
 *   d     = min(0.993, (1 + t) / (10 + t));  the kernel receives float(1 - d)                        (model.py:126-127:
 *           num_updates = global_step read AFTER the increment -- one reading of the control dependency)
 * Per element, float32, contraction off, each operation rounded once, in this order:
 *   1. g' = g + weight_decay * w  if the tensor decays (add_weight_decay, model.py:132-145: its name contains "weights" or
 *      "kernel" and does not contain "depthwise_weights"), else g' = g
 *   2. m += (g' - m) * one_minus_beta1            one_minus_beta1 = float(0.1)
 *   3. v += (g' * g' - v) * one_minus_beta2       one_minus_beta2 = float(0.001)
 *   4. w -= (m * alpha) / (sqrt(v) + epsilon)     epsilon = 1e-8f OUTSIDE the bias correction (TF's "epsilon hat"); sqrt and the
 *      division correctly rounded, denormals kept
 *   5. ema -= (ema - w) * one_minus_decay         with the new w
 * A tensor whose grad pointer is NULL (torch: p.grad is None; TF: a None gradient) keeps w, m and v; its ema still takes step 5.
 * m and v start at 0, ema as a copy of w (the caller's initialisation).  A numpy float32 restatement is bit-exact.
 *
 * The table: T rows, one per tensor.  tensors_host is read by this call to refuse bad rows; tensors_dev holds the same rows in
 * device memory (8-byte aligned), which the kernel reads -- the caller's upload, ordered before this call on `stream`.  A tensor
 * is cut into blocks of SSD_UPDATE_BLOCK_ELEMS elements counted from the 16-byte boundary at or below w:
 *   blocks(row) = ceil((count + ((uintptr_t)w / 4) % 4) / SSD_UPDATE_BLOCK_ELEMS),   first_block = sum of blocks(rows before it)
 * (the caller fills first_block; this call checks it).  w, m, v, ema and grad need 4-byte alignment only: where the five
 * addresses are congruent modulo 16 the tensor moves as 16-byte loads and stores with a scalar head and tail, otherwise element
 * by element; the result bits are the same.  The tensors must not overlap.  No LDS, no atomics, no allocation, no host
 * synchronisation: the call only enqueues one kernel on `stream` and is legal during stream capture.
 * NULL tables, T < 1 or > SSD_UPDATE_MAX_TENSORS, tensors_dev not 8-byte aligned, a negative count or one above 2^40, a NULL or
 * misaligned w / m / v / ema, a misaligned grad, a decay flag other than 0 / 1, a wrong first_block, more than 2^31 - 1 blocks,
 * or a non-finite scalar: SSD_ERR_INVALID before any HIP call.  Needs no handle. */
#define SSD_UPDATE_BLOCK_ELEMS 4096
#define SSD_UPDATE_MAX_TENSORS 65536
typedef struct ssd_update_tensor {           /* 56 bytes, no padding */
    float *w;                                /* the variable                                                   */
    const float *grad;                       /* its gradient, or NULL: only ema moves                          */
    float *m, *v;                            /* Adam's first and second moment                                 */
    float *ema;                              /* the variable's moving average                                  */
    int64_t count;                           /* elements                                                       */
    int32_t decay;                           /* 1: step 1 adds weight_decay * w                                */
    int32_t first_block;                     /* blocks of the rows before this one (see above)                 */
} ssd_update_tensor;
typedef struct ssd_update_scalars {          /* 24 bytes: this step's scalars, all finite                      */
    float alpha, one_minus_beta1, one_minus_beta2, epsilon, weight_decay, one_minus_decay;
} ssd_update_scalars;
int ssd_train_update(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T,
                     const ssd_update_scalars *scalars, void *stream);

/* ---- the TRAIN step's norms: sum w^2, sum g^2 and the non-finite counts of every tensor of the update's table ----
 *
 * What a training loop reports and checks every step (tf.estimator's total_loss holds weight_decay * sum l2_loss(K), model.py:80-81;
 * NanTensorHook stops a run whose loss is not finite), for a whole model in TWO launches over the table ssd_train_update takes, run
 * BEFORE the update.  The table, its rows, the first_block rule and every refusal are the TRAIN update's (above); m, v and ema are
 * validated as there and never dereferenced; w and grad are read and never written.  Outputs, in device memory, rows in table order:
 *   sums [T][2] double:  sum over the tensor of w^2, of grad^2      bad [T][2] int64:  non-finite elements of w, of grad
 * Arithmetic: an element's square is formed in double, where it is exact ((double)x * (double)x, 48 significant bits); a non-finite
 * element (NaN, +inf, -inf) contributes +0.0 to its sum and 1 to its count.  A NULL grad gives sum g^2 = +0.0 and bad g = 0.
 * Order of the double additions, fixed here so that a numpy float64 restatement is bit-exact:
 *   The work list is the update's: blocks of SSD_UPDATE_BLOCK_ELEMS VIRTUAL elements counted from the 16-byte boundary at or below
 *   w; virtual element j of a tensor is its element j - pad, pad = ((uintptr_t)w / 4) % 4 ALWAYS (whatever the alignment of grad:
 *   grad's element i is taken with w's element i); the tensor is the virtual elements [pad, pad + count).
 *   Stage 1, one partial per block, j0 the block's first virtual element: lane t of 256 owns the virtual elements
 *   j0 + (k * 256 + t) * 4 + e, k = 0..3 outer, e = 0..3 inner, and adds the squares of those inside the tensor in that order,
 *   starting from +0.0.  The 256 lane values a[t] are then added by the binary tree a[t] += a[t + s] for t < s, s = 128, 64, ..., 1;
 *   a[0] is the block's partial.  (How the tree is carried out -- cross-lane moves, LDS -- is free, as long as it is this tree.)
 *   Stage 2: a tensor's value is its blocks' partials added in ascending block order, starting from +0.0; a row of no blocks
 *   gives +0.0 and 0.  Counts are integers.  No atomics anywhere: two calls give the same bits, and the bits do not depend on
 *   which load width moved an element.
 * workspace: ssd_train_norms_workspace_bytes(tensors_host, T) = 32 bytes per block of the table (two doubles and two int64 per
 * block; 0 for a table of empty tensors and for a table the call would refuse), 16-byte aligned, written by stage 1 and read by
 * stage 2; its contents need no initialisation.  No allocation, no host synchronisation: the call only enqueues two kernels
 * on `stream` (one when the table has no blocks) and is legal during stream capture.  Beyond the update's refusals (without the
 * scalars): a NULL sums or bad or one not 8-byte aligned, a NULL workspace or one not 16-byte aligned, a workspace smaller than
 * the planner's figure: SSD_ERR_INVALID before any HIP call.  Needs no handle. */
#define SSD_NORMS_BLOCK_BYTES 32
size_t ssd_train_norms_workspace_bytes(const ssd_update_tensor *tensors_host, int32_t T);
int ssd_train_norms(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, double *sums,
                    int64_t *bad, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the TRAIN step's histograms: tf.summary.histogram of every variable and of every gradient of total_loss ----
 *
 * What train.py's summaries show of a run (model.py:121-123: `<name>_hist`, `<name>_grad_hist`), for a whole model in THREE launches
 * over the table ssd_train_update takes, run BEFORE the update.  TensorFlow's sources are not available to this project: the rule
 * below restates histogram::Histogram with its default limits from memory; what is pinned is this rule, NOT parity with TensorFlow.
 * The table, its rows, the first_block rule and every refusal are the TRAIN update's; m, v and ema are validated and never
 * dereferenced; w and grad are read and never written.
 * Limits: start v = 1e-12 (double); while v < 1e20 append v and set v *= 1.1 (one double multiplication each); then append DBL_MAX.
 *   The table is the negated list reversed, then 0.0, then the list: NB entries, strictly increasing, antisymmetric about its middle.
 *   ssd_histogram_limits(out, capacity) returns NB and fills out[0 .. NB) when out != NULL and capacity >= NB (else it writes
 *   nothing): the ONE definition -- the caller uploads exactly this table once and passes it as limits_dev.
 * Planes: plane 0 of a row is w; plane 1 is the gradient of total_loss, g' = g + weight_decay * w where decay == 1, else g' = g (one
 *   fp32 multiply and one fp32 add, contraction off: step 1 of ssd_train_update).  A NULL grad gives an all-zero plane 1 with num = 0.
 * Bucket of a finite element x: widen x to double; the bucket is the index of the first limit strictly greater than it (upper_bound:
 *   the number of limits <= x; -0.0 goes with +0.0).  A non-finite element (NaN, +inf, -inf) counts in `bad` and enters no bucket and
 *   no statistic.
 * Outputs, in device memory, rows in table order; the caller need not clear them:
 *   counts [T][2][NB] int64     stats [T][2] ssd_histogram_stats: sum of (double)x, sum_squares of (double)x * (double)x, min, max,
 *   num (the finite elements) and bad.  min and max order -0.0 below +0.0 (so that they do not depend on the order of the elements);
 *   of a plane without a finite element they are +inf and -inf.
 * Order of the double additions: exactly the TRAIN step's norms' (above) -- the virtual elements from the 16-byte boundary at or
 *   below w (pad taken from w, whatever grad's alignment), lane t's 16 elements k outer, e inner from +0.0, the 256-lane tree
 *   a[t] += a[t + s], the blocks' partials in ascending order from +0.0; an element outside the tensor or not finite adds +0.0.  A
 *   numpy float64 restatement is bit-exact; stats[t][0].sum_squares has the bits of ssd_train_norms' sums[t][0], and
 *   stats[t][1].sum_squares those of sums[t][1] where decay == 0.
 * Atomics: the bucket counts are integers and are added with integer atomics (LDS inside a block, vector global atomics for a
 *   block's flush); they change no bit: two calls give the same bytes.  No floating-point atomics.  The process-wide option
 *   "hist_scheme" (ssd_set_option(NULL, ...)) picks how a wave's equal buckets meet the LDS atomic: -1 the library's choice (1) | 0
 *   one atomic per element | 1 one ballot: a wave whose finite elements all share one bucket adds their number once, any other wave
 *   takes one atomic per element | 2, 3: one, two rounds in which the lanes that share the first pending lane's bucket are counted
 *   with a ballot and added by one lane, then one atomic per remaining element | 4 and above: rounds until nothing is pending.
 *   The results are the same bytes under every value.
 * workspace: ssd_train_histograms_workspace_bytes(tensors_host, T) = SSD_HISTOGRAM_BLOCK_BYTES per block of the table (0 for a table
 * of empty tensors and for one the call would refuse), 16-byte aligned, written by stage 1 and read by stage 2, no initialisation.
 * No allocation, no host synchronisation: the call only enqueues on `stream` (a clear of counts, stage 1 unless the table has no
 * blocks, stage 2).  Beyond the update's refusals (without its scalars): a NULL limits_dev, counts or stats or one not 8-byte
 * aligned, a NULL workspace or one not 16-byte aligned, a workspace smaller than the planner's figure, a non-finite weight_decay:
 * SSD_ERR_INVALID before any HIP call.  Needs no handle. */
#define SSD_HISTOGRAM_BLOCK_BYTES 64
#define SSD_HISTOGRAM_STATS_BYTES 40
typedef struct ssd_histogram_stats {         /* 40 bytes, no padding */
    double sum, sum_squares;                 /* of the finite elements, in double                              */
    float min, max;                          /* of the finite elements; +inf, -inf when there is none          */
    int64_t num, bad;                        /* finite elements; NaN and +-inf                                 */
} ssd_histogram_stats;
int32_t ssd_histogram_limits(double *out, int32_t capacity);
size_t ssd_train_histograms_workspace_bytes(const ssd_update_tensor *tensors_host, int32_t T);
int ssd_train_histograms(const ssd_update_tensor *tensors_host, const ssd_update_tensor *tensors_dev, int32_t T, float weight_decay,
                         const double *limits_dev, int64_t *counts, ssd_histogram_stats *stats, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- the TRAIN step's gradient exchange: every rank's gradients gathered once and summed in rank order ----
 *
 * Data-parallel training over G ranks (one process per GPU) without an all-reduce, whose order of additions would depend on the
 * backend, its ring and the world size: every rank PACKS its gradients, its moving statistics and a 3-word header into one slice
 * of a receive buffer, the caller runs ONE all-gather of the slices (any backend: the bytes are what matters), and every rank
 * REDUCES the G slices in ascending rank order back into its own tensors.  Every rank computes the same bits from the same bytes.
 * The reference has no multi-GPU code; the loss rule below is its loss (ssd.py:121-133) over the global batch.
 *
 * The table: T rows (1 .. SSD_UPDATE_MAX_TENSORS), one per tensor; rows_host is read by the call to refuse bad rows, rows_dev holds
 * the same rows in device memory (8-byte aligned), which the kernel reads -- the caller's upload, ordered before the call on `stream`.
 *   data     the tensor: read by pack, written by reduce; 4-byte aligned.  NULL: pack ships +0.0 for the row and reduce writes
 *            nothing (a parameter without a gradient).  The data ranges of a table must not overlap.
 *   count    elements, 0 .. 2^40
 *   offset   the row's first float in the payload (below)
 *   kind     0: a gradient, weighted by c_r | 1: a moving statistic, the plain mean over the ranks
 * The bucket layout depends on the counts alone, so it is the same on every rank whatever the addresses are:
 *   offset_0 = 0,  offset_{t+1} = offset_t + roundup(count_t, 4);   payload floats P = roundup(offset_T, SSD_UPDATE_BLOCK_ELEMS)
 *   a slice = SSD_REDUCE_HEADER_FLOATS header floats, then the payload: ssd_train_bucket_floats(rows_host, T) = 16 + P floats
 *   (0 for a table the calls would refuse).  Header word 0: this rank's matches n_r (a float), word 1: its localization loss, word 2:
 *   its classification loss, words 3 .. 15: +0.0.  The gathered buffer is [G][16 + P] floats, 16-byte aligned, rank r's slice at r.
 * ssd_train_grad_pack writes EVERY float of one slice: the header (header_dev: 3 floats in device memory), each row's elements at its
 *   offset, and +0.0 for a row's padding to 4, for a NULL row and for the payload behind the last row -- the collective never ships
 *   an uninitialised byte.  The values are copied, bit for bit.
 * ssd_train_grad_reduce reads gathered[G][16 + P].  float32, contraction off, every operation rounded once, max(a, 1) = a > 1 ? a : 1:
 *   S   = n_0 + n_1 + ... + n_{G-1}, added in ascending order
 *   c_r = max(n_r, 1) / max(S, 1), the division correctly rounded                                       -> weights_out[r]
 *   kind 0:  acc = x_0 * c_0;  acc = acc + x_r * c_r  for r = 1 .. G-1;  data[i] = acc
 *   kind 1:  acc = x_0;        acc = acc + x_r        for r = 1 .. G-1;  data[i] = acc * (1.0f / (float)G)
 *   losses_out[0], [1]: the kind-0 rule on header words 1 and 2 (the losses over the global batch, normalised by max(S, 1), when
 *   every rank's loss is normalised by its own max(n_r, 1))
 *   At G = 1, c_0 = 1.0f and x * 1.0f keeps every bit of x (-0.0, denormals, a quiet NaN's payload): the exchange is the identity.
 *   A NaN an operation creates (inf - inf) is some quiet NaN: its sign and payload are not pinned, and neither is the payload that
 *   survives where two NaNs meet.  A numpy float32 restatement is otherwise bit-exact.  No atomics: two calls give the same bytes, and the
 *   bits do not depend on whether an element moved in a 16-byte group (data 16-byte aligned) or alone (any other alignment).
 * Both calls only enqueue one kernel on `stream` (256 lanes, blocks of SSD_UPDATE_BLOCK_ELEMS bucket floats, a grid of at most 2048
 * striding over them): no LDS, no allocation, no host synchronisation, no handle.  SSD_ERR_INVALID before any HIP call: NULL tables
 * or buffers; rows_dev not 8-byte, slice / gathered not 16-byte, header_dev / losses_out / weights_out / data not 4-byte aligned;
 * T out of range; a negative count or one above 2^40; an offset other than the rule's; a kind other than 0 / 1; G < 1 or
 * G > SSD_REDUCE_MAX_RANKS; slice_floats other than ssd_train_bucket_floats(rows_host, T); data ranges that overlap. */
#define SSD_REDUCE_HEADER_FLOATS 16
#define SSD_REDUCE_MAX_RANKS 16
typedef struct ssd_reduce_row {              /* 32 bytes, no padding */
    float *data;                             /* the tensor, or NULL: zeros out, nothing back                   */
    int64_t count;                           /* elements                                                       */
    int64_t offset;                          /* first float of the row in the payload (see above)              */
    int32_t kind;                            /* 0: weighted by c_r | 1: plain mean                             */
    int32_t reserved;
} ssd_reduce_row;
int64_t ssd_train_bucket_floats(const ssd_reduce_row *rows_host, int32_t T);
int ssd_train_grad_pack(const ssd_reduce_row *rows_host, const ssd_reduce_row *rows_dev, int32_t T, const float *header_dev,
                        float *slice, int64_t slice_floats, void *stream);
int ssd_train_grad_reduce(const ssd_reduce_row *rows_host, const ssd_reduce_row *rows_dev, int32_t T, const float *gathered,
                          int32_t G, int64_t slice_floats, float *losses_out, float *weights_out, void *stream);

/* ---- the TRAIN head: forward and backward of RetinaNetBoxPredictor in TRAIN mode (box_predictor.py:34-155) ----
 *
 * The predictor is ten dense 3x3 stride-1 'same' convolutions (two towers of four 256 -> 256 layers shared by the pyramid
 * levels, then `logits` and `encoded_boxes` with a bias), each tower layer followed by a per-level training-mode batch norm and
 * a ReLU (layer_utils.py:5-12).  These calls are those two operations and their gradients.  Conventions as for the loss,
 * augment and update blocks: device pointers of the caller, logical NHWC fp32 tensors and HWIO kernels, DEVICE weights (they
 * change every step), scratch from a caller-supplied workspace, every call only enqueues on `stream` (no allocation, no host
 * round trip, no synchronisation), arguments are refused with SSD_ERR_INVALID before any HIP call, no handle.  No atomics
 * anywhere: two calls give the same bits.  Not here: strides other than 1 and 1x1 kernels (the TRAIN FPN block below), depthwise
 * backward (the TRAIN backbone block below), F16X3, double backward.
 *
 * A convolution call takes 1 .. SSD_TRAIN_MAX_LEVELS levels that share B, Cin, Cout and ONE kernel; the weight gradient is the
 * sum over all of them.  Cin must be a multiple of 8, Cin and Cout at most 4096, every level's tensors (channels padded to 32)
 * below 2 GiB.  x, dy, out, w_dev, dw_dev and the workspace need 16-byte alignment, bias_dev / dbias_dev 4-byte.
 * The implicit-GEMM launches follow the PROCESS-wide kernel selectors of ssd_set_option(NULL, ...) ("igemm_96", "igemm_tile",
 * "igemm_deep64"), like the handle-less stage entry points; none changes a result bit, but "igemm_96" changes the padded width
 * and with it the workspace size: size the workspace under the options the call will run with (a call re-plans and refuses a
 * workspace that has become too small).
 *
 * ssd_conv3x3_train_forward   out_l = conv3x3_same(x_l, w) (+ bias), raw.  The kernel is packed on the device into ssd_conv2d's
 *   layout and the launch is ssd_conv2d's exact-fp32 implicit GEMM: per output ONE fmaf chain over taps row-major, ci ascending
 *   within a tap, then + bias -- bit-identical to ssd_conv2d on the same values.
 * ssd_conv3x3_train_backward  from x_l, dy_l, w:
 *   dx_l (levels[l].out; given for every level or for none)  = conv3x3_same(dy_l, w'), w'[kh,kw,co,ci] = w[2-kh,2-kw,ci,co], on the
 *     same launch: ONE fmaf chain over taps row-major, co ascending within a tap -- bit-identical to the CPU oracle's
 *     conv2d(dy, w').  Widths that are not multiples of 32 on the reduction side are zero padded.
 *   dw_dev [3,3,Cin,Cout] = sum over levels, images and positions of x (shifted by the tap, zero outside) * dy, on
 *     v_mfma_f32_32x32x2_f32.  Order (this implementation's, deterministic, NOT pinned to an oracle chain): the positions of a
 *     level are cut into slices of rows_per_slice consecutive rows r = (b * H + y) * W + x (rows_per_slice = the total row count
 *     over max(1, 1536 / tiles) slices, tiles = 9 * ceil(Cin / 128) * ceil(Cout / (Cout <= 32 ? 32 : 128)), at least 256,
 *     rounded up to 16); within a slice one fp32 chain in ascending r; the slices' partial tiles, kept in the workspace, are
 *     then added one fp32 addition at a time in ascending slice order, levels in list order.
 *   dbias_dev [Cout] (nullable) = sum of dy over everything, in double in the two-stage order of the batch norm below over the
 *     concatenated levels, rounded once.
 *
 * The batch norm takes 1 .. SSD_TRAIN_MAX_LEVELS levels x [rows, C] (rows = B*H*W) with their OWN parameters and statistics
 * (per-level batch norms, box_predictor.py:41-45); C <= 1024; every pointer 16-byte aligned.  Fixed two-stage order of every
 * column sum: with G = ceil(min(C, 1024) / 4), rpp = 256 / G and slab_rows = max(8 * rpp, ceil(total rows of the call / 1024)) rounded up to
 * a multiple of rpp, a level's rows are cut into slabs of slab_rows; inside a slab row lane j = (r - slab start) mod rpp adds its
 * rows in ascending order, the lanes are added in ascending j, the slabs in ascending order; all in double, rounded ONCE.
 * ssd_bn_relu_train_forward, training != 0:
 *     mean = fp32(sum x / rows);  var = fp32(sum (x - mean)^2 / rows), difference and square in double (biased)
 *     invstd = 1 / sqrt(var + epsilon), two correctly rounded fp32 operations
 *     out = max(((x - mean) * (gamma * invstd)) + beta, 0), one fp32 operation at a time, no contraction
 *     mean / invstd (required) and var (nullable) receive the batch statistics; where the moving statistics are given
 *       moving_mean -= (moving_mean - mean) * one_minus_momentum
 *       moving_variance -= (moving_variance - var * fp32(rows / (rows - 1))) * one_minus_momentum     (rows == 1: var itself)
 *     (TF's fused batch norm restated from memory: unpinned against TensorFlow, like the update block's formulas.)
 *   training == 0: out = max(((x - moving_mean) * (gamma * (1 / sqrt(moving_variance + epsilon)))) + beta, 0), the inference form
 *     ssd_finalize folds into ssd_conv2d's epilogue; nothing else is written and the workspace is not used.
 * ssd_bn_relu_train_backward, with t = x - mean, xhat = t * invstd, sf = gamma * invstd, y = t * sf + beta RECOMPUTED from x and the
 *   saved statistics (the forward's output is not read), g = y > 0 ? dy : 0:
 *     dbeta = fp32(sum g), dgamma = fp32(sum g * xhat) (products and sums in double)
 *     out = sf * ((g - dbeta / rows) - xhat * (dgamma / rows)), one fp32 operation at a time, rows as fp32 */
#define SSD_TRAIN_MAX_LEVELS 8
typedef struct ssd_conv_level {              /* 32 bytes */
    int32_t H, W;                            /* the level's INPUT size (TRAIN head: input == output)            */
    const float *x;                          /* [B,H,W,Cin]: the layer's input                                   */
    const float *dy;                         /* backward: [B,H,W,Cout] upstream gradient; forward: not read      */
    float *out;                              /* forward: [B,H,W,Cout]; backward: dx [B,H,W,Cin] or NULL          */
} ssd_conv_level;
typedef struct ssd_bn_level {                /* 104 bytes */
    int64_t rows;                            /* B*H*W                                                            */
    const float *x;                          /* [rows, C]: the batch norm's input                                */
    const float *dy;                         /* backward: [rows, C]                                              */
    float *out;                              /* forward: y; backward: dx                                         */
    const float *gamma, *beta;               /* [C]                                                              */
    float *moving_mean, *moving_variance;    /* [C], nullable as a pair in training (then not updated)           */
    float *mean, *var, *invstd;              /* [C]: written by the training forward, mean / invstd read by the backward */
    float *dgamma, *dbeta;                   /* [C]: backward                                                    */
} ssd_bn_level;
/* Bytes of workspace either convolution call needs for these sizes (0: the sizes would be refused); pointers are not read. */
size_t ssd_conv3x3_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout);
int ssd_conv3x3_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                              const float *w_dev /* [3,3,Cin,Cout] */, const float *bias_dev /* [Cout] or NULL */,
                              void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_conv3x3_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                               const float *w_dev, float *dw_dev /* [3,3,Cin,Cout] */, float *dbias_dev /* [Cout] or NULL */,
                               void *workspace_dev, size_t workspace_bytes, void *stream);
/* Bytes of workspace either batch-norm call needs (0: refused sizes); only `rows` of the levels is read. */
size_t ssd_bn_relu_train_workspace_bytes(const ssd_bn_level *levels, int32_t n_levels, int32_t C);
int ssd_bn_relu_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t training, float epsilon,
                              float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_bn_relu_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, void *workspace_dev,
                               size_t workspace_bytes, void *stream);

/* ---- the TRAIN FPN: forward and backward of fpn() in TRAIN mode on a frozen backbone (feature_extractor.py:40-76) ----
 *
 * fpn() is ten dense convolutions on 256 output channels and five batch norms + ReLU:
 *     x5 = lateral5(c5) (1x1)                p5 = conv3x3(x5)
 *     x4 = lateral4(c4) + up2(x5)            p4 = conv3x3(x4)          up2 = nearest-neighbour x2 upsampling
 *     x3 = lateral3(c3) + up2(x4)            p3 = conv3x3(x3)
 *     p6 = conv3x3 stride 2 (c5)             p7 = conv3x3 stride 2 (relu(p6)), the RAW p6: the batch norms come last (:71-74)
 * The batch norms are the TRAIN head's calls above.  The convolutions are the TRAIN head's pair with three more arguments, under
 * the TRAIN head's conventions (caller's device pointers, logical NHWC fp32, HWIO kernels in device memory, caller's workspace,
 * SSD_ERR_INVALID before any HIP call, enqueue only, no atomics: two calls give the same bits).  The six ssd_conv3x3_train_* /
 * ssd_bn_relu_train_* entry points ARE these calls with k = 3, stride = 1, up_dev = NULL: same planner, same launches, same bits.
 *
 *   k       1 or 3.  pad_beg = 0 for k = 1, 1 for k = 3.
 *   stride  1 or 2; 2 only with k = 3.  In ssd_conv_level H, W are the INPUT's size; the output (out of the forward, dy of the
 *           backward) is H x W for stride 1 and ceil(H/2) x ceil(W/2) for stride 2: conv2d_same's explicit pad of 1 before and
 *           1 after with a 'valid' convolution (layer_utils.py:25-43).  Backward: out = dx is [B,H,W,Cin].
 *   up_dev  forward only, nullable: n_levels pointers, up_dev[l] = [B,H/2,W/2,Cout] added to level l's output after nearest x2
 *           upsampling.  Only with stride 1, even H and W, bias_dev == NULL, every entry non-NULL and 16-byte aligned.
 * Cin: a multiple of 8 for k = 3, of 4 for k = 1 (ShuffleNet's c3 has 116 channels); Cin, Cout <= 4096; every level's tensors
 * (channels padded to 32) below 2 GiB.  ssd_conv_train_workspace_bytes sizes the workspace of either call (with_up != 0: a forward
 * that will pass up_dev); 0 for refused sizes.
 *
 * ssd_conv_train_forward    out_l = conv(x_l, w) (+ bias) (+ up2(up_l)) on ssd_conv2d's exact-fp32 implicit GEMM with the kernel
 *   packed on the device: bit-identical to ssd_conv2d with the same k, stride, pad_beg and up_dev -- per output ONE fmaf chain
 *   over taps row-major, ci ascending within a tap, then one fp32 addition of the bias or of the upsampled value.
 * ssd_conv_train_backward
 *   dw_dev [k,k,Cin,Cout] on v_mfma_f32_32x32x2_f32: tap (kh,kw) of output position (oy,ox) multiplies
 *     x[oy*stride + kh - pad_beg, ox*stride + kw - pad_beg] (zero outside the input) with dy[oy,ox]; the sum runs over the levels,
 *     images and OUTPUT positions.  Order: the TRAIN head's slice rule with 9 replaced by k*k and the rows counted at the output --
 *     rows_per_slice = the total OUTPUT row count over max(1, 1536 / tiles) slices, tiles = k*k * ceil(Cin / 128) *
 *     ceil(Cout / (Cout <= 32 ? 32 : 128)), at least 256, rounded up to 16; a level's output rows r = (b * OH + oy) * OW + ox are
 *     cut into such slices, one fp32 chain in ascending r within a slice, the slices added one fp32 addition at a time in
 *     ascending order, levels in list order.  k = 3, stride 1 is the TRAIN head's order and bits.  This implementation's order,
 *     deterministic, NOT pinned to an oracle chain.
 *   dx (levels[l].out, for every level or for none):
 *     k = 3, stride 1   as the TRAIN head's.
 *     k = 3, stride 2   dx = conv3x3_same(D, w') on the same launch, D [B,H,W,Cout] with D[b,2oy,2ox,:] = dy[b,oy,ox,:] and zero
 *                       elsewhere (written into the workspace by the step that permutes dy), w' the TRAIN head's rotated,
 *                       transposed kernel.  Consequence: ONE fmaf chain per element over taps row-major, co ascending within a
 *                       tap, the zeros of D included -- on finite data bit-identical to the CPU oracle's conv2d(D, w').
 *     k = 1             REFUSED with a non-NULL out: nothing trainable lies upstream of a lateral while the backbone is frozen.
 *   dbias_dev (nullable; the FPN has no bias) as the TRAIN head's, over the output rows.
 *
 * ssd_fpn_merge_backward   the backward of the top-down merge and of the ReLU between p6 and p7, one streaming kernel:
 *     same_size == 0   out[b,y,x,c] = base[b,y,x,c] + g[b,2y,2x,c] + g[b,2y,2x+1,c] + g[b,2y+1,2x,c] + g[b,2y+1,2x+1,c]
 *                      with g [B,2H,2W,C]: dx4 = dx4' + (the 2x2 sums of dx3)
 *     same_size != 0   out[b,y,x,c] = base[b,y,x,c] + g[b,y,x,c] with g [B,H,W,C]: d p6 = d p6' + relu'(p6) * dx(p7's input)
 *   fp32, added left to right as written, no contraction.  base_dev NULL: the sum starts at +0.  gate_dev [B,H,W,C] nullable: where
 *   gate > 0 is false (zero of either sign, negative, NaN) every g term of that element reads as +0 (the g value is not used: a
 *   NaN there does not spread).  out, base, gate are [B,H,W,C]; out_dev may be base_dev (in place), no other overlap.  16-byte
 *   accesses where C % 4 == 0, element-wise otherwise; every pointer 16-byte aligned.  B <= 65536, H, W <= 16384, C <= 4096. */
size_t ssd_conv_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                      int32_t k, int32_t stride, int32_t with_up);
int ssd_conv_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout, int32_t k,
                           int32_t stride, const float *w_dev /* [k,k,Cin,Cout] */, const float *bias_dev /* [Cout] or NULL */,
                           const float *const *up_dev /* NULL or [n_levels] */, void *workspace_dev, size_t workspace_bytes,
                           void *stream);
int ssd_conv_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout, int32_t k,
                            int32_t stride, const float *w_dev, float *dw_dev /* [k,k,Cin,Cout] */,
                            float *dbias_dev /* [Cout] or NULL */, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_fpn_merge_backward(const float *base_dev, const float *g_dev, const float *gate_dev, int32_t B, int32_t H, int32_t W,
                           int32_t C, int32_t same_size, float *out_dev, void *stream);

/* ---- the TRAIN backbone: forward and backward of MobileNet-v1's Conv2d_1 .. Conv2d_13 in TRAIN mode (mobilenet_v1.py:52-67) ----
 *
 * Each of the 13 blocks is a 3x3 depthwise convolution ('SAME', stride 1 or 2) and a 1x1 convolution, each followed by a
 * training-mode batch norm and ReLU6.  These calls are the operations the TRAIN head and the TRAIN FPN lack for it: the raw
 * depthwise convolution with its two gradients, the data gradient of a 1x1 convolution, and the batch norm with ReLU6.  Conv2d_0
 * (3 -> 32, stride 2) stays FROZEN BY DEFAULT: it then runs through ssd_first_conv on its moving statistics; its own forward and
 * weight gradient are the block "the TRAIN first convolution" below.
 * Conventions as for the TRAIN head: the caller's device pointers, logical NHWC fp32, TF-layout kernels in DEVICE memory, the
 * caller's workspace, SSD_ERR_INVALID before any HIP call, enqueue only, no atomics: two calls give the same bits.  Every existing
 * entry point keeps its arguments, its refusals and its bits (ssd_conv_train_backward still refuses dx with k = 1).  Not here:
 * F16X3, double backward; ShuffleNet's split and shuffle are the block "the TRAIN ShuffleNet" below.
 *
 * The depthwise calls: x [B,H,W,C], w_dev [3,3,C,1] (= [9][C]), out / dy [B,OH,OW,C] with OH = ceil(H / stride), OW likewise, and
 * pad_beg = p = max((OH - 1) * stride + 3 - H, 0) / 2 (TF 'SAME': 1 for stride 1; for stride 2, 0 on even and 1 on odd sizes).
 * C a multiple of 4; stride 1 or 2; stride 2 with H and W of different parity is refused (one pad_beg serves both axes); B <= 65536,
 * H, W <= 32768, B*H*W < 2^31, fewer than 2^40 elements; every pointer 16-byte aligned.
 *
 * ssd_depthwise_train_forward   raw tf.nn.depthwise_conv2d: ssd_depthwise3x3's kernel on the caller's device weights without batch
 *   norm and activation -- per output ONE fmaf chain from +0 over the taps row-major, a tap outside the input contributing
 *   fmaf(0, w, acc): bit-identical to ssd_depthwise3x3 (no batch norm, no activation) and to the CPU oracle's depthwise3x3.
 * ssd_depthwise_train_backward  (C <= 1024) from x, dy, w:
 *   dx_dev [B,H,W,C] (nullable)   dx[b,iy,ix,c] = sum of dy[b,(iy+p-ky)/s,(ix+p-kx)/s,c] * w[ky,kx,c] over the taps whose source
 *     index is an integer inside the output.  Order: ONE fmaf chain per element from +0 over the taps of the flipped kernel
 *     row-major, i.e. ky = 2, 1, 0 and within each kx = 2, 1, 0; taps without a source are SKIPPED.  On finite data that is
 *     bit-identical to the CPU oracle's depthwise3x3(E, flip(w), stride 1), E [B,H,W,C] zero except E[b,s*oy+1-p,s*ox+1-p,:] =
 *     dy[b,oy,ox,:] (stride 1: E = dy): a chain that starts at +0 never holds -0, so the oracle's fmaf(0, w, acc) is acc.  E is
 *     never materialised.
 *   dw_dev [3,3,C,1]   dw[ky,kx,c] = sum over b, oy, ox of x[b,oy*s+ky-p,ox*s+kx-p,c] * dy[b,oy,ox,c] (positions outside the input
 *     contribute nothing): 9 * C column sums over the OUTPUT rows r = (b * OH + oy) * OW + ox, products and sums in double, rounded
 *     ONCE.  Fixed two-stage order, the batch norm's: with G = C / 4, rpp = 256 / G and slab_rows = max(8 * rpp,
 *     ceil(B*OH*OW / 1024)) rounded up to a multiple of rpp, the rows are cut into slabs of slab_rows; inside a slab row lane
 *     j = (r - slab start) mod rpp adds its rows in ascending order, the lanes are added in ascending j, the slabs in ascending
 *     order.  The partial sums ([slabs][9][C] doubles) live in the workspace.
 *
 * ssd_pointwise_train_backward  ssd_conv_train_backward with k = 1 that also gives the data gradient: levels, B, Cin, Cout, w_dev
 *   [1,1,Cin,Cout] and dw_dev as there (Cin a multiple of 4; dw_dev: the same launches and bits); dx goes to levels[l].out, for
 *   every level or for none: dx_l = conv1x1(dy_l, w'), w'[0,0,co,ci] = w[0,0,ci,co] packed on the device, on the forward's exact-fp32
 *   implicit GEMM: ONE fmaf chain per element, co ascending -- bit-identical to the CPU oracle's conv2d(dy, w').  The reduction
 *   side (Cout) is zero padded to a multiple of 32.  ssd_pointwise_train_workspace_bytes sizes its workspace (0: refused sizes).
 *
 * ssd_bn_act_train_forward / _backward are ssd_bn_relu_train_forward / _backward with one more argument, act = SSD_ACT_RELU or
 * SSD_ACT_RELU6 (anything else is refused); the old pair IS these calls with SSD_ACT_RELU: same planner, same launches, same bits,
 * and ssd_bn_relu_train_workspace_bytes sizes both.  With SSD_ACT_RELU6:
 *     forward    out = min(max(y, 0), 6) as v = y > 0 ? y : 0; v = v < 6 ? v : 6 (the inference path's activation), y as above;
 *                training == 0 is the epilogue ssd_finalize folds into the engine's layers, bit for bit
 *     backward   g = (y > 0 && y < 6) ? dy : 0 with y recomputed from x and the saved statistics; the rest as above
 *   A NaN y gives out = 0 and a closed gate; y == 6 closes the gate as y == 0 does (TF's Relu6Grad restated from memory: unpinned
 *   against TensorFlow, like the batch norm's formulas above). */
int ssd_depthwise_train_forward(const float *x_dev, int32_t B, int32_t H, int32_t W, int32_t C, const float *w_dev /* [3,3,C,1] */,
                                int32_t stride, float *out_dev, void *stream);
/* Bytes of workspace ssd_depthwise_train_backward needs (0: the sizes would be refused). */
size_t ssd_depthwise_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride);
int ssd_depthwise_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                                 const float *w_dev, int32_t stride, float *dx_dev /* nullable */, float *dw_dev /* [3,3,C,1] */,
                                 void *workspace_dev, size_t workspace_bytes, void *stream);
size_t ssd_pointwise_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout);
int ssd_pointwise_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                 const float *w_dev /* [1,1,Cin,Cout] */, float *dw_dev, void *workspace_dev, size_t workspace_bytes,
                                 void *stream);
int ssd_bn_act_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, int32_t training, float epsilon,
                             float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_bn_act_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, void *workspace_dev,
                              size_t workspace_bytes, void *stream);

/* ---- the TRAIN first convolution: forward and weight gradient of Conv2d_0 (3 -> Cout, 3x3, stride 2) from uint8 frames ----------
 *
 * The layer the TRAIN backbone leaves frozen BY DEFAULT (mobilenet_v1.py:34-50: slim.conv2d on the normalised frames, 'SAME', then
 * batch norm and ReLU6; ShuffleNet's Conv1 is the same convolution with 24 channels).  These calls are its raw convolution and its
 * weight gradient; its batch norm + ReLU6 are ssd_bn_act_train_forward / _backward above.  There is no data gradient: the input is
 * the image.  Conventions are the TRAIN backbone's: the caller's device pointers, the TF-layout kernel [3,3,3,Cout] (= [27][Cout],
 * row t = (ky * 3 + kx) * 3 + ci) in DEVICE memory, the caller's workspace, SSD_ERR_INVALID with the argument named in
 * ssd_last_error() before any HIP call, enqueue only, no synchronisation, no atomics: two calls give the same bits.
 *
 * images_dev [B,H,W,3] uint8 at the network's own size (no resize), H and W even; out / dy [B,H/2,W/2,Cout]; Cout a multiple of 4,
 * at most 64; B*H*W*3 < 2^31 (so R = B * (H/2) * (W/2) < 2^31); float pointers and the workspace 16-byte aligned, images_dev 4-byte
 * aligned.  The pixel value is the inference path's: with inv255 = (float)(1.0 / 255.0), p(u) = fp32(2 * fp32(u * inv255) - 1), no
 * contraction (the oracle's preprocess).  TF 'SAME' on even sizes has pad_beg = 0: output (oy,ox) reads rows 2oy .. 2oy+2 and
 * columns 2ox .. 2ox+2; row H (ky = 2 on the last output row) and column W (kx = 2 on the last output column) are outside the input.
 *
 * ssd_first_conv_train_forward   raw, no batch norm, no activation: ssd_first_conv's kernels on the caller's device weights -- per
 *   output ONE fmaf chain from +0 over the taps row-major, ci ascending within a tap, a tap outside the input contributing
 *   fmaf(0, w, acc): bit-identical to ssd_first_conv without batch norm and activation and to the CPU oracle's
 *   conv2d(preprocess(images), w, stride 2).
 * ssd_first_conv_train_backward  from the images and dy:
 *   dw_dev [3,3,3,Cout]   dw[ky,kx,ci,co] = sum over b, oy, ox of p(images[b,2oy+ky,2ox+kx,ci]) * dy[b,oy,ox,co] (positions outside the
 *     input contribute nothing): 27 * Cout column sums over the OUTPUT rows r = (b * OH + oy) * OW + ox, OH = H/2, OW = W/2, products
 *     and sums in double (the product of two floats is exact in double), rounded ONCE.  Fixed two-stage order, the batch norm's with
 *     C = Cout: with G = Cout / 4, rpp = 256 / G and slab_rows = max(8 * rpp, ceil(R / 1024)) rounded up to a multiple of rpp, the
 *     rows are cut into slabs of slab_rows; inside a slab row lane j = (r - slab start) mod rpp adds its rows in ascending order,
 *     the lanes are added in ascending j, the slabs in ascending order.  The partial sums ([slabs][27][Cout] doubles) live in the
 *     workspace, which ssd_first_conv_train_workspace_bytes sizes (0: the sizes would be refused).
 * Not here: a resize in front of the convolution (TRAIN batches arrive at the network's size); ShuffleNet's max pool has its gradient in
 * the block "the TRAIN ShuffleNet" below. */
int ssd_first_conv_train_forward(const uint8_t *images_dev, int32_t B, int32_t H, int32_t W, const float *w_dev /* [3,3,3,Cout] */,
                                 int32_t Cout, float *out_dev, void *stream);
size_t ssd_first_conv_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout);
int ssd_first_conv_train_backward(const uint8_t *images_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t Cout,
                                  float *dw_dev /* [3,3,3,Cout] */, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the TRAIN first convolution from float frames: the same layer on float32 [B,H,W,3] images in [0, 1] -------------------------
 *
 * What Pipeline(is_training=True) / ssd_augment yield and the reference's backbones take (mobilenet_v1.py:10-11,34 and
 * shufflenet_v2.py: x = 2.0 * images - 1.0): frames after crop, resize, colour offsets, grayscale and the random scale, which are
 * NOT on the byte grid.  Conventions are those of the block above: the caller's device pointers, the TF-layout kernel [3,3,3,Cout]
 * in DEVICE memory, the caller's workspace, SSD_ERR_INVALID with the argument named in ssd_last_error() before any HIP call,
 * enqueue only, no synchronisation, no atomics: two calls give the same bits.
 *
 * images_dev [B,H,W,3] float32 NHWC at the network's own size, H and W even; out / dy [B,H/2,W/2,Cout]; Cout a multiple of 4, at
 * most 64; every float pointer and the workspace 16-byte aligned.  The kernels address the frames through a buffer resource with
 * 32-bit byte offsets: B*H*W*12 < 2^31 bytes (312 frames of 640 x 896); a larger batch is refused and the workspace call returns
 * 0 for it.
 *
 * The pixel value is q(x) = fp32(2 * x - 1): 2 * x is exact, so ONE rounding; no contraction, no clamp, no special case -- what
 * the pipeline clipped to [0, 1] stays there, anything else goes through as IEEE arithmetic takes it.  Consequence: for
 * x = fp32(u * inv255), the first step of ssd_augment, q(x) is the block above's p(u) bit for bit, so frames on the byte grid
 * give the uint8 calls' results, forward and dw.
 *
 * ssd_first_conv_f32_train_forward   raw, no batch norm, no activation: per output ONE fmaf chain from +0 over the taps
 *   row-major, ci ascending within a tap, a tap outside the input (row H, column W) contributing fmaf(0, w, acc): bit-identical
 *   to the CPU oracle's conv2d(q(images), w, stride 2) with q computed in fp32.
 * ssd_first_conv_f32_train_backward  from the images and dy:
 *   dw_dev [3,3,3,Cout]   dw[ky,kx,ci,co] = sum over b, oy, ox of q(images[b,2oy+ky,2ox+kx,ci]) * dy[b,oy,ox,co], positions outside
 *     the input contributing nothing: products and sums in double, rounded ONCE, in the two-stage slab order of
 *     ssd_first_conv_train_backward with C = Cout (the same slab_rows, lanes and slabs), partial sums [slabs][27][Cout] doubles
 *     in the workspace, which ssd_first_conv_f32_train_workspace_bytes sizes by the same formula (0: the sizes would be refused).
 * There is no data gradient.  Not here: a resize, NCHW frames, quantising the floats back to bytes. */
int ssd_first_conv_f32_train_forward(const float *images_dev, int32_t B, int32_t H, int32_t W, const float *w_dev /* [3,3,3,Cout] */,
                                     int32_t Cout, float *out_dev, void *stream);
size_t ssd_first_conv_f32_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cout);
int ssd_first_conv_f32_train_backward(const float *images_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t Cout,
                                      float *dw_dev /* [3,3,3,Cout] */, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the TRAIN ShuffleNet: what ShuffleNet-v2 in TRAIN mode needs beyond the TRAIN backbone (shufflenet_v2.py:9-135) --------------
 *
 * ShuffleNet-v2 is Conv1 (the first convolution with 24 channels, batch norm + ReLU), a 3x3 stride-2 max pool, three stages of
 * units and Conv5.  A unit works on channel halves: 1x1 convolution + batch norm + ReLU, 3x3 depthwise + batch norm WITHOUT an
 * activation, 1x1 + batch norm + ReLU; between units concat_shuffle_split interleaves the two halves and splits them again, and a
 * stage closes with a concat.  At depth_multiplier 1.0 the Stage2 halves have 58 channels.  These calls are what the TRAIN blocks
 * above refuse or lack for it: channel counts that are even but no multiple of 4, the batch norm without an activation, the
 * shuffle and the concat with their gradients, and the gradient of the max pool (the forward stays ssd_maxpool3x3s2, which only
 * enqueues).  Conventions are the TRAIN backbone's: the caller's device pointers, logical NHWC fp32, TF-layout kernels in DEVICE
 * memory, the caller's workspace, SSD_ERR_INVALID with the argument named in ssd_last_error() before any HIP call, enqueue only
 * (no allocation, no synchronisation, no host round trip, no index table), no atomics: two calls give the same bits.  Every
 * pointer 16-byte aligned.  The entry points above keep their arguments, their refusals and their bits; these share their
 * planners and kernels.  ONE thing changes for the older calls too: the batch-norm kernels (ssd_bn_relu_train_*, ssd_bn_act_train_*,
 * dbias) and the weight gradient of ssd_conv*_train_backward / ssd_pointwise_train_backward now read and write rows whose width is
 * 2 mod 4 (C = 6, a Cout of 58) 8 bytes at a time where they went element by element -- the same values in the same order, so no
 * result bit moves, and the 16-byte alignment they already require covers it.  Not here: depth_multiplier 2.0 (Conv5's 2048 channels: the batch norm takes 1024), F16X3, the fusion of a
 * shuffle or concat into its neighbouring convolutions.
 *
 * ssd_sn_depthwise_train_forward / _workspace_bytes / _backward   ssd_depthwise_train_* with C any EVEN number (C <= 1024 for the
 *   backward; odd C is refused): the same fmaf chains (forward: taps row-major from +0, a tap outside contributing fmaf(0, w, acc);
 *   dx: the flipped kernel's taps, those without a source skipped) and the same double column sums of dw, the slab rule written for
 *   G = ceil(C / 4) quads (rpp = 256 / G; C = 58: G = 15, rpp = 17, slab_rows >= 136; the last quad's second pair lies outside the
 *   tensor).  C % 4 == 0: the old entry points' launches and bits.  C % 4 == 2: the same kernels instantiated for 2 channels per
 *   lane -- every access is 8 bytes (a row of 58 floats is 232 bytes, so every row start and every channel pair is 8-byte aligned);
 *   no access falls to 4 bytes.
 * ssd_sn_pointwise_train_forward / _workspace_bytes / _backward   a 1x1 stride-1 convolution with Cin and Cout any EVEN numbers up
 *   to 4096, levels as in ssd_conv_train_*.  forward: ssd_conv_train_forward with k = 1 (no bias, no upsample-add), bit-identical
 *   to ssd_conv2d with k = 1 on the same values.  backward: ssd_pointwise_train_backward -- dx (levels[l].out, for every level or
 *   for none) ONE fmaf chain per element, co ascending, bit-identical to the CPU oracle's conv2d(dy, w'); dw by the k = 1 slice
 *   rule of the TRAIN FPN.  Both reduction sides are zero padded to a multiple of 32 by the steps that permute x / dy and pack the
 *   kernel (element-wise, any width); the weight gradient loads x and dy rows 16 bytes at a time where the width is a multiple of
 *   4, 8 bytes where it is even.  Cin % 4 == 0: the old calls' launches and bits.
 * ssd_sn_bn_train_forward / _backward   ssd_bn_act_train_forward / _backward that also take act = SSD_ACT_NONE: forward out = y,
 *   backward g = dy; the rest of the float32 sequence of the TRAIN head's batch norm is unchanged, and training == 0 is the
 *   inference form (x - moving_mean) * sf + beta, bit for bit what ssd_finalize folds behind the engine's depthwise layers.
 *   SSD_ACT_RELU / SSD_ACT_RELU6: the old pair's planner, launches and bits.  ssd_bn_relu_train_workspace_bytes sizes all of them.
 *   Rows of C % 4 == 2 channels are read and written 8 bytes at a time.
 *
 * ssd_sn_shuffle_train   on [rows, D] tensors, rows >= 1, 1 <= D <= 2^20, rows * D < 2^39 (the limits of all four copies).
 *   transpose == 0   concat_shuffle_split (shufflenet_v2.py:94-115): z[2i] = x[i], z[2i+1] = y[i] (i < D); xo = z[:D], yo = z[D:].
 *   transpose != 0   its backward: x_dev, y_dev hold the gradients of xo and yo, dz = [x | y], and xo_dev, yo_dev receive those of x
 *                    and y: xo[i] = dz[2i], yo[i] = dz[2i+1].
 * ssd_sn_concat_train   out [rows, 2D] = [x | y], the stage's closing tf.concat (shufflenet_v2.py:89);  ssd_sn_split_train its
 *   backward: dx = g[:, :D], dy = g[:, D:].
 *   All four are pure copies of 32-bit words: every bit pattern arrives unchanged, NaN payloads and -0 included.  Indices are
 *   computed arithmetically.  Accesses are 16-byte where D % 4 == 0, 8-byte where D % 2 == 0, else element-wise.  No tensor read
 *   may overlap a tensor written, nor two written ones each other (refused).
 *
 * ssd_sn_maxpool_train_backward   the gradient of ssd_maxpool3x3s2 (3x3, stride 2, 'SAME' on even H and W: pad_beg = 0, window
 *   (oy,ox) covers rows 2oy .. 2oy+2 and columns 2ox .. 2ox+2, cells beyond the edge take no part): x [B,H,W,C], dy [B,H/2,W/2,C],
 *   dx [B,H,W,C]; C a multiple of 4 (at least 4), H and W even (at least 2), as the forward; B <= 65536, H, W <= 32768, B*H*W < 2^31,
 *   fewer than 2^40 elements; dx_dev may alias neither x_dev nor dy_dev.  A gather, no atomics: an input position lies in at most four
 *   windows, and dx[b,iy,ix,c] is the sum of dy over those windows in which this position is the WINNER, one fp32 addition at a time
 *   from +0 over the won windows in ascending (oy, ox).  The winner of a window is the FIRST tap in row-major order whose value
 *   equals the window's forward output, m = a > m ? a : m from -inf over the taps row-major (NaN taps never replace m); a window
 *   whose output equals none of its taps (all NaN) gives its gradient to nobody.  (TF's MaxPoolGrad tie rule restated from memory:
 *   unpinned against TensorFlow, like the batch norm's formulas above.) */
int ssd_sn_depthwise_train_forward(const float *x_dev, int32_t B, int32_t H, int32_t W, int32_t C, const float *w_dev /* [3,3,C,1] */,
                                   int32_t stride, float *out_dev, void *stream);
size_t ssd_sn_depthwise_train_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride);
int ssd_sn_depthwise_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C,
                                    const float *w_dev, int32_t stride, float *dx_dev /* nullable */, float *dw_dev /* [3,3,C,1] */,
                                    void *workspace_dev, size_t workspace_bytes, void *stream);
/* Bytes of workspace either pointwise call needs (0: the sizes would be refused). */
size_t ssd_sn_pointwise_train_workspace_bytes(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout);
int ssd_sn_pointwise_train_forward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                   const float *w_dev /* [1,1,Cin,Cout] */, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_sn_pointwise_train_backward(const ssd_conv_level *levels, int32_t n_levels, int32_t B, int32_t Cin, int32_t Cout,
                                    const float *w_dev, float *dw_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_sn_bn_train_forward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, int32_t training, float epsilon,
                            float one_minus_momentum, void *workspace_dev, size_t workspace_bytes, void *stream);
int ssd_sn_bn_train_backward(const ssd_bn_level *levels, int32_t n_levels, int32_t C, int32_t act, void *workspace_dev,
                             size_t workspace_bytes, void *stream);
int ssd_sn_shuffle_train(const float *x_dev, const float *y_dev, int64_t rows, int32_t D, int32_t transpose, float *xo_dev,
                         float *yo_dev, void *stream);
int ssd_sn_concat_train(const float *x_dev, const float *y_dev, int64_t rows, int32_t D, float *out_dev, void *stream);
int ssd_sn_split_train(const float *g_dev, int64_t rows, int32_t D, float *dx_dev, float *dy_dev, void *stream);
int ssd_sn_maxpool_train_backward(const float *x_dev, const float *dy_dev, int32_t B, int32_t H, int32_t W, int32_t C, float *dx_dev,
                                  void *stream);

/* ---- the COCO box matching: CocoBoxEval.evaluate() of coco_metric.py for every cell of a run in one launch ----
 *
 * The reference scores val2017 with pycocotools' COCOeval (inference/evaluate_on_COCO.ipynb cell 17); coco_metric.py restates it,
 * and its evaluate() -- computeIoU + evaluateImg per (category, area range, image) -- is what this call computes, bit for bit.
 * These semantics are coco_metric.py's, read off its code; this block is their single statement for the kernel, for
 * tests/helpers/coco_match_ref.py and for the Python that packs and unpacks (coco_match.py).
 *
 * A cell is one (category, image) pair with at least one detection or groundtruth box.  The packed arrays hold the cells' rows
 * back to back; cell c owns detections [det_begin, det_begin + D) and groundtruth boxes [gt_begin, gt_begin + G).
 *   detections    arrive ordered and truncated: descending score, ties in input order (np.argsort(-scores, kind="mergesort")), the
 *                 first SSD_COCO_MAX_DET.  Each carries its xywh box (four float64) and its area (float64, float(bbox[2] * bbox[3])
 *                 as the constructor forms it: passed in, not recomputed).  Scores stay on the host.
 *   groundtruth   arrives in annotation order: an xywh box (float64), an area (float64) and a crowd byte (non-zero: crowd).
 * IoU(d, g): float64, one IEEE operation at a time, no contraction:
 *   w = min(dx + dw, gx + gw) - max(dx, gx),  h = min(dy + dh, gy + gh) - max(dy, gy)
 *   !(w > 0 && h > 0):  iou = +0.0
 *   else  inter = w * h,  da = dw * dh,  ga = gw * gh,  union = crowd ? da : (da + ga) - inter,  iou = inter / union
 *   (bbox_iou of coco_metric.py, bit for bit: the division is correctly rounded).
 * Area range a with bounds (lo, hi) = area_rng_host[a]:
 *   ig[g] = crowd[g] || area[g] < lo || area[g] > hi
 *   the scan order of the groundtruth boxes: all !ig boxes in annotation order, then all ig boxes in annotation order (the stable
 *   sort by the flag); gt_ignore of the cell is the flags in that order.
 * Threshold t: thr_host[t], the caller's float64 values (coco_metric.THR_L), never recomputed.
 * The scan of (a, t), for the detections d in order:
 *   best = thr, m = none
 *   for g in scan order:
 *     skip g if it is taken and not crowd
 *     stop if m is set, !ig[m] and ig[g]
 *     skip g if iou(d, g) < best
 *     best = iou(d, g), m = g                 (an equal IoU moves the match to the later box)
 *   if m is set: matched[t, d] = 1, ignored[t, d] = ig[m], m becomes taken
 *   afterwards: ignored[t, d] |= !matched[t, d] && (darea[d] < lo || darea[d] > hi)
 * A cell without groundtruth gives matched = 0 and ignored = out of range; a cell without detections gives only gt_ignore.
 * All inputs are finite (the caller checks; the call cannot, they are device memory).
 *
 * Outputs: matched_dev / ignored_dev uint16 [A, nd], bit t of element [a, det_begin + d] = matched / ignored [t, d] of the cell at
 * area range a (bits from T on are 0); gt_ignore_dev uint8 [A, ng], 0 / 1, the cell's flags in SCAN order at [a, gt_begin ..];
 * iou_dev (nullable; a test aid) float64, cell after cell the [D, G] matrix in ANNOTATION order: cell c's block starts at the sum
 * of D * G over the cells before it.  Every element that belongs to a cell is written; rows of no cell are left alone.
 *
 * The call only enqueues one kernel on `stream` (256 lanes, one wave per cell, SSD_COCO_CELLS_PER_BLOCK cells per block, a grid
 * of at most SSD_COCO_GRID_CAP blocks striding over the cells): no allocation, no synchronisation, no atomics, no handle; two calls
 * give the same bits.  cells_host is read by the call to refuse bad cells, cells_dev holds the same rows in device memory (8-byte
 * aligned), which the kernel reads -- the caller's upload, ordered before the call on `stream`.  n_cells == 0 enqueues nothing.
 * SSD_ERR_INVALID before any HIP call, the reason naming the argument: a NULL thr_host / area_rng_host; NULL cells with n_cells > 0;
 * a NULL array whose count (nd or ng) is positive; a pointer not aligned to its element; n_cells, nd or ng outside [0, 2^40]; T outside
 * [1, SSD_COCO_MAX_THR]; A outside [1, SSD_COCO_MAX_AREA]; T * A > 64; a cell with D outside [0, SSD_COCO_MAX_DET] or G outside
 * [0, SSD_COCO_MAX_GT]; detection or groundtruth ranges that are not ascending and disjoint, or that run past nd / ng. */
#define SSD_COCO_MAX_DET 100                 /* MAX_DETS[-1] of coco_metric.py                                  */
#define SSD_COCO_MAX_GT 256                  /* groundtruth boxes of one cell; larger cells stay on the host   */
#define SSD_COCO_MAX_THR 16
#define SSD_COCO_MAX_AREA 4
#define SSD_COCO_CELLS_PER_BLOCK 4
#define SSD_COCO_GRID_CAP 1024               /* blocks; the rest of the cell list is grid-strided               */
typedef struct ssd_coco_cell {               /* 24 bytes, no padding */
    int64_t det_begin, gt_begin;             /* first row of the cell in the detection / groundtruth arrays    */
    int32_t D, G;                            /* detections, groundtruth boxes                                  */
} ssd_coco_cell;
int ssd_coco_match(const ssd_coco_cell *cells_host, const ssd_coco_cell *cells_dev, int64_t n_cells,
                   const double *det_box_dev /* [nd,4] */, const double *det_area_dev /* [nd] */, int64_t nd,
                   const double *gt_box_dev /* [ng,4] */, const double *gt_area_dev, const uint8_t *gt_crowd_dev, int64_t ng,
                   const double *thr_host /* [T] */, int32_t T, const double *area_rng_host /* [A,2] */, int32_t A,
                   uint16_t *matched_dev /* [A,nd], bit t */, uint16_t *ignored_dev /* [A,nd] */,
                   uint8_t *gt_ignore_dev /* [A,ng], scan order */, double *iou_dev /* nullable: cell-major [D,G], annotation order */,
                   void *stream);

/* ---- the COCO accumulation: CocoBoxEval.accumulate() of coco_metric.py for every (category, area range, maxDets) in one launch ----
 *
 * accumulate() merges the cells of a category by descending score and reads the precision / recall curves off the cumulative
 * counts.  These semantics are coco_metric.py's, read off its code; this block is their single statement for the kernel
 * (csrc/coco_accumulate.hip), for tests/helpers/coco_accumulate_ref.py and for the Python that packs (coco_accumulate.py).
 *
 * Rows.  The rows are the packed detections of ssd_coco_match: cells category-major with the image ascending, inside a cell at most
 *   SSD_COCO_MAX_DET detections in descending score (what coco_match.pack produces).  nd < 2^31.
 * Segments.  One ssd_coco_segment per category k, in cat_ids order: the category's consecutive rows [det_begin, det_begin +
 *   det_count) of the detection arrays and [gt_begin, gt_begin + gt_count) of gt_ignore.  A category with no cell has both counts 0.
 * Row inputs.
 *   order_dev  int32 [nd]: order[p] is the packed row at global position p.  Global order: ascending category, then descending
 *              score, then ascending packed row -- the host's stable argsort(-sc, kind="mergesort") over the concatenation in image
 *              order.  Scores stay on the host, which computes the order (one np.lexsort); positions [det_begin, det_begin +
 *              det_count) of segment k hold exactly that category's rows.  An element outside [0, nd) is never read through.
 *   rank_dev   uint8 [nd]: a row's position inside its cell, 0 .. SSD_COCO_MAX_DET - 1.
 * Matching inputs.  matched_dev / ignored_dev uint16 [A, nd], bit t; gt_ignore_dev uint8 [A, ng]: exactly ssd_coco_match's outputs.
 * Settings.  max_dets_host int32 [M], positive and ascending; rec_thr_host float64 [R], ascending and finite, the caller's values
 *   (coco_metric.REC_THRS), never recomputed; rec_thr_dev the same values in device memory.  T <= SSD_COCO_MAX_THR,
 *   A <= SSD_COCO_MAX_AREA, M <= SSD_COCO_MAX_MAXDETS, R <= SSD_COCO_MAX_REC.
 * Per (k, a):  npig = the number of zero bytes among the category's gt_ignore[a, ..].  npig == 0: precision[:, :, k, a, :] and
 *   recall[:, k, a, :] are -1.0.
 * Per (k, a, m, t) with npig > 0:  the participating rows are the category's rows in global order with rank < max_dets[m], j = 0 .. n - 1.
 *   tp_j = rows <= j with matched && !ignored,  fp_j = rows <= j with !matched && !ignored  (integers; an ignored row participates
 *   and changes no count)
 *   float64, one IEEE operation at a time, every division correctly rounded, eps = 2^-52:
 *     rc_j = double(tp_j) / double(npig),   pr_j = double(tp_j) / ((double(fp_j) + double(tp_j)) + eps)
 *   E_j = max(pr_j, .., pr_(n-1))
 *   recall[t, k, a, m] = rc_(n-1), +0.0 for n == 0
 *   precision[t, r, k, a, m] = E_pos with pos the first j with rc_j >= rec_thr[r]; +0.0 if there is none, or if n == 0
 *   rc_j depends on tp_j alone and is monotone in it, so with c_r the smallest integer c >= 0 with
 *   double(c) / double(npig) >= rec_thr[r], pos is the first j with tp_j >= c_r -- the row where tp steps to c_r -- and row 0 when
 *   c_r == 0; there is none when c_r > tp_(n-1).  This is the form the kernel uses.  (After a real matching tp_(n-1) <= npig, every
 *   true positive holding a box of its own, so a c_r above npig never has a row; the kernel does not rely on it.)
 * Outputs.  precision_dev float64 [T, R, K, A, M], recall_dev float64 [T, K, A, M], the host arrays' C order; every element is written.
 *
 * The call only enqueues one kernel on `stream` (256 lanes, one wave per (k, a, m), SSD_COCO_CELLS_PER_BLOCK of them per block, a
 * grid of at most SSD_COCO_GRID_CAP blocks striding over the list): no allocation, no synchronisation, no atomics, no handle, no
 * scratch; two calls give the same bits.  segments_host is read by the call to refuse bad rows, segments_dev holds the same rows in
 * device memory (8-byte aligned) -- the caller's upload, ordered before the call on `stream`.  K == 0 enqueues nothing.
 * SSD_ERR_INVALID before any HIP call, the reason "ssd_coco_accumulate: ..." naming the argument: a NULL max_dets_host /
 * rec_thr_host; NULL segments, rec_thr_dev, precision_dev or recall_dev with K > 0; a NULL array whose count (nd or ng) is positive;
 * a pointer not aligned to its element; T outside [1, SSD_COCO_MAX_THR]; A outside [1, SSD_COCO_MAX_AREA]; M outside
 * [1, SSD_COCO_MAX_MAXDETS]; R outside [1, SSD_COCO_MAX_REC]; K outside [0, 2^20]; nd outside [0, 2^31 - 1]; ng outside [0, 2^40];
 * max_dets not positive and ascending; rec_thr not finite and ascending; a segment with a negative count; detection ranges that do
 * not tile [0, nd) in order (det_begin of the first segment 0, of every other the end of the one before, the last end nd);
 * groundtruth ranges that are not ascending and disjoint, or that run past ng. */
#define SSD_COCO_MAX_MAXDETS 4
#define SSD_COCO_MAX_REC 128
typedef struct ssd_coco_segment {            /* 32 bytes, no padding: the rows of one category                 */
    int64_t det_begin, det_count;            /* its positions of order_dev = its rows of the detection arrays  */
    int64_t gt_begin, gt_count;              /* its elements of every row of gt_ignore_dev                     */
} ssd_coco_segment;
int ssd_coco_accumulate(const ssd_coco_segment *segments_host, const ssd_coco_segment *segments_dev, int32_t K,
                        const int32_t *order_dev /* [nd] */, const uint8_t *rank_dev /* [nd] */,
                        const uint16_t *matched_dev /* [A,nd], bit t */, const uint16_t *ignored_dev /* [A,nd] */, int64_t nd,
                        const uint8_t *gt_ignore_dev /* [A,ng] */, int64_t ng, int32_t T, int32_t A,
                        const int32_t *max_dets_host /* [M] */, int32_t M,
                        const double *rec_thr_host /* [R] */, const double *rec_thr_dev /* [R] */, int32_t R,
                        double *precision_dev /* [T,R,K,A,M] */, double *recall_dev /* [T,K,A,M] */, void *stream);

/* ---- the COCO rows: the detections of ssd_coco_match built from the engine's record blocks, for every image in two launches ----
 *
 * The dict route turns a record into ssd_coco_match's rows in four host steps: ssd.score_filter, coco_eval.detection_records,
 * CocoBoxEval.__init__ and coco_match.pack.  These two calls are those four steps for all images at once; the semantics are that
 * Python's, read off its code; this block is their single statement for the kernel (csrc/coco_rows.hip) and for
 * coco_rows.rows_host, the same function in numpy.
 *
 * Records.  records_dev holds n_images records of ssd_record_words() = 6T + 1 32-bit words each, back to back:
 *   boxes [T,4] f32 (ymin, xmin, ymax, xmax, normalised) | scores [T] f32 | labels [T] i32 | num_boxes i32.
 *   Image i is record i, row i of image_hw_dev and column i of the [K, n_images] tables; the caller orders the images by ascending
 *   id, so a flattened [K, n_images] table is in coco_match.pack's cell order (category ascending, then image ascending).
 *   image_hw_dev int32 [n_images, 2]: height, width of the ORIGINAL image (positive; float(height) is what the boxes are scaled by).
 *   label_to_cat_dev int32 [num_labels]: the index of the label's category in cat_ids, or -1 for a category that is not evaluated
 *   (a value outside [-1, K) counts as -1).
 * Row semantics.  Only rows j < num_boxes exist; the words behind them are never read into a result.  In float32, every operation
 *   rounded on its own (no fused multiply-add):
 *     kept     score > (float)score_threshold                       (strict; what numpy does for scores[:n] > 0.15)
 *     py0 = ymin * H, px0 = xmin * W, py1 = ymax * H, px1 = xmax * W      (H = (float)height, W = (float)width)
 *     x = trunc(px0), y = trunc(py0), w = trunc(px1 - px0), h = trunc(py1 - py0)     (toward zero)
 *   and then x, y, w, h as float64, area = (double)((int64)w * (int64)h), score = (double)score.
 *   k = label_to_cat[label]; a kept row with k == -1 is dropped.
 *   A row is BAD if its score is not finite, or if it is kept and its label lies outside [0, num_labels) or one of its four products
 *   is not below 2^30 in magnitude (a NaN, an infinity, or a box no image holds).  A bad row is dropped.
 *   bad[i] = the lowest bad row of image i, or -1; T if num_boxes lies outside [0, T] (the image then has no rows).  The caller
 *   raises on bad[i] != -1 -- the role coco_match._finite plays on the dict route -- so rows of such an image may hold anything.
 * Order within a cell.  The rows of one (category, image) cell are ordered by descending score, ties by ascending record row; the
 *   first SSD_COCO_MAX_DET are kept.  rank(j) = #{j' kept, same category : s' > s or (s' == s and j' < j)}.
 * ssd_coco_rows_count writes counts[k, i] = min(rows of the cell, SSD_COCO_MAX_DET) for every k, zeros included, and bad[i].
 * ssd_coco_rows_fill recomputes the ranks and writes the row of rank r < SSD_COCO_MAX_DET at det_begin[k, i] + r of det_box_dev
 *   (xywh), det_area_dev and det_score_dev; det_begin is the exclusive scan of the flattened counts, nd its total.  A position
 *   outside [0, nd) is not written; rows of no cell are left alone.
 *
 * Each call only enqueues one kernel on `stream` (256 lanes, one wave per image, SSD_COCO_CELLS_PER_BLOCK images per block, a grid
 * of at most SSD_COCO_GRID_CAP blocks striding over the images, 32 * T bytes of LDS per block): no allocation, no synchronisation,
 * no atomics, no handle; two calls give the same bits.  The 32-byte box row is stored as two 16-byte stores when det_box_dev is
 * 16-byte aligned, else as four 8-byte stores.  n_images == 0 enqueues nothing, and neither does a fill with nd == 0.
 * SSD_ERR_INVALID before any HIP call, the reason "ssd_coco_rows_count: ..." / "ssd_coco_rows_fill: ..." naming the argument:
 * n_images outside [0, 2^31 - 1]; T outside [1, SSD_COCO_ROWS_MAX_T]; K outside [1, 2^20]; K * n_images > 2^31 - 1; num_labels
 * outside [1, 2^20]; a score_threshold that is not finite; nd outside [0, 2^31 - 1]; with n_images > 0 a NULL records_dev,
 * image_hw_dev, label_to_cat_dev, counts_dev, bad_dev or det_begin_dev, and with nd > 0 too a NULL det_box_dev, det_area_dev or
 * det_score_dev; a pointer not aligned to its element (4 bytes, 8 for det_begin_dev and the three row arrays). */
#define SSD_COCO_ROWS_MAX_T 2048             /* rows of one record: two words of LDS per row and wave, 64 KB per block; the    */
                                             /* reference's configs have T = 80 classes * 25 boxes = 2000                     */
int ssd_coco_rows_count(const int32_t *records_dev, int64_t n_images, int32_t T,
                        const int32_t *image_hw_dev /* [n_images,2] */, const int32_t *label_to_cat_dev /* [num_labels] */,
                        int32_t num_labels, int32_t K, float score_threshold,
                        int32_t *counts_dev /* [K,n_images] */, int32_t *bad_dev /* [n_images] */, void *stream);
int ssd_coco_rows_fill(const int32_t *records_dev, int64_t n_images, int32_t T,
                       const int32_t *image_hw_dev /* [n_images,2] */, const int32_t *label_to_cat_dev /* [num_labels] */,
                       int32_t num_labels, int32_t K, float score_threshold,
                       const int64_t *det_begin_dev /* [K,n_images] */, int64_t nd,
                       double *det_box_dev /* [nd,4] xywh */, double *det_area_dev /* [nd] */, double *det_score_dev /* [nd] */,
                       void *stream);

/* ---- the VOC-style metric: coco_eval.Evaluator.evaluate() (train.py's evaluation metric) in two launches ----
 *
 * coco_eval.average_precision walks the detections of one label in descending confidence and decides, one after the other, which
 * are true positives.  Whether a detection is one depends only on the detections and groundtruth boxes of its own (label, image)
 * and on their relative order; the order over all images is needed only for the cumulative counts.  So: ssd_voc_match decides
 * every (label, image) cell on its own, ssd_voc_curve walks each label's rows once.  These semantics are coco_eval.py's, read off
 * its code; this block is their single statement for the two kernels (csrc/voc_match.hip), for tests/helpers/voc_match_ref.py and
 * for the Python that packs (voc_match.py).
 *
 * Rows.  A row is a detection: a label, an image, an insertion index (the order the detections were added in), a float64
 *   confidence and a float64 box (ymin, xmin, ymax, xmax).  The global order is ascending label, then descending confidence, then
 *   ascending insertion index (list.sort / the stable argsort(-conf) of every label).  A row's place in it is its `pos`; the rows
 *   of a label are consecutive.  n_rows < 2^31.
 * Cells.  A cell is the rows of one (label, image), in global order, with the groundtruth boxes of that label and image in
 *   insertion order.  The packed arrays hold the cells' rows back to back: cell c owns detections [det_begin, det_begin + D) of
 *   det_box / det_pos and groundtruth boxes [gt_begin, gt_begin + G) of gt_box; det_pos[i] is the pos of packed detection i.
 * IoU(d, g): float64, one IEEE operation at a time, no contraction, the division correctly rounded (_iou_matrix of coco_eval.py):
 *   w = min(d.xmax, g.xmax) - max(d.xmin, g.xmin),  h = min(d.ymax, g.ymax) - max(d.ymin, g.ymin)
 *   inter = w * h if w > 0 and h > 0, else +0.0
 *   a_d = (d.xmax - d.xmin) * (d.ymax - d.ymin), a_g alike;  iou = inter / ((a_d + a_g) - inter) if inter > 0, else +0.0
 *   All inputs are finite and no product overflows (the caller checks finiteness; the calls cannot, they are device memory).
 * The scan of a cell, for its detections in order:
 *   best = the FIRST groundtruth box with the maximal IoU (a strict > in insertion order)
 *   the detection is a true positive iff iou[best] > 0, iou[best] >= thr and best is not taken; it then takes best and records
 *   iou[best].  A cell with G = 0 has no true positive.
 *   On the GPU lane l looks at the boxes l + 64 * j in ascending j and keeps its first maximum; the wave takes the exact maximum of
 *   the 64 lane maxima and, among the lanes that hold it, the smallest box index -- the first maximum of the cell.  Lane l keeps
 *   `taken` of its boxes as bit j of one 64-bit mask: SSD_VOC_MAX_GT = 64 * 64 boxes per cell; larger cells stay on the host.
 * The curve of a label over its rows k = 0 .. n - 1 in global order, with num_gt = max(groundtruth boxes of the label, 1):
 *   ctp_k = true positives among rows 0 .. k (integers);  P_k = double(ctp_k) / double(k + 1),  R_k = double(ctp_k) / double(num_gt)
 *   best_index = the first k that maximises (P_k * R_k) * (1.0 - |P_k - R_k|); precision, recall = P, R there; best_threshold = the
 *     confidence of that row
 *   ap = the sum, from +0.0 in ascending k, of P_k * (R_k - double(ctp_k - 1) / double(num_gt)) for a true positive, +0.0 otherwise
 *   iou_sum = the sum, in the same order, of the recorded IoUs (+0.0 for the others);  mean_iou = iou_sum / double(max(tp, 1))
 *   n = 0: every field is 0.
 *   (R_k - R_(k-1) is exactly that difference for a true positive and 0 otherwise; every term is >= +0.0, so the +0.0 terms and the
 *   +0.0 a lane past the end contributes change no bit.  The host forms ap with np.sum's pairwise order instead: the two agree
 *   within rounding, every other field bit for bit.)
 *
 * ssd_voc_match: one wave per cell, SSD_VOC_CELLS_PER_BLOCK cells per block of 256 lanes, a grid of at most SSD_VOC_GRID_CAP blocks
 * striding over the cells.  Writes tp_dev[det_pos[i]] (0 / 1) and tp_iou_dev[det_pos[i]] (the recorded IoU, +0.0 unless a true
 * positive) for every packed detection i, cells with G = 0 included; an element whose index is not in det_pos is left alone (the
 * caller's host fallback of an oversize cell lives there), and a det_pos outside [0, n_rows) is never stored through.  With
 * nd == n_rows and det_pos a permutation every element of both outputs is written.
 * ssd_voc_curve: one wave per label, the same block and grid shape, over segments {begin, count, num_gt}: the label's rows are
 * [begin, begin + count) of tp_dev / tp_iou_dev / conf_dev (the confidences in global order).  64 rows at a time: ctp from one
 * ballot and a running carry, a running first maximum per lane (the final reduction takes the larger value and, of equal values,
 * the smaller index), the two ordered sums as chains of dependent additions in ascending lane order.  Writes one ssd_voc_result
 * per label, all 64 bytes.
 *
 * Both calls only enqueue one kernel on `stream`: no allocation, no synchronisation, no atomics, no handle; two calls give the same
 * bits.  cells_host / segments_host are read by the call to refuse bad rows; cells_dev / segments_dev hold the same rows in device
 * memory (8-byte aligned) -- the caller's upload, ordered before the call on `stream`.  n_cells == 0 / n_labels == 0 enqueues nothing.
 * SSD_ERR_INVALID before any HIP call, the reason "<fn>: ..." naming the argument:
 *   ssd_voc_match   n_cells, nd or ng outside [0, 2^40]; n_rows outside [0, 2^31 - 1]; nd > n_rows; a thr that is not finite; NULL cells
 *                   with n_cells > 0; a NULL array whose count is positive; a pointer not aligned to its element; a cell with D < 0
 *                   or G outside [0, SSD_VOC_MAX_GT]; detection ranges that do not tile [0, nd) in order (det_begin of the first
 *                   cell 0, of every other cell the end of the cell before, the last end nd); groundtruth ranges that are not
 *                   ascending and disjoint or run past ng.
 *   ssd_voc_curve   n_labels outside [0, 2^24]; n_rows outside [0, 2^31 - 1]; NULL segments or results with n_labels > 0; a NULL array
 *                   with n_rows > 0; a pointer not aligned to its element; a segment with count < 0, begin < 0, begin + count past
 *                   n_rows, or num_gt outside [1, 2^40]. */
#define SSD_VOC_MAX_GT 4096                  /* groundtruth boxes of one cell: 64 lanes x one 64-bit mask      */
#define SSD_VOC_CELLS_PER_BLOCK 4
#define SSD_VOC_GRID_CAP 1024                /* blocks; the rest of the cell / label list is grid-strided      */
typedef struct ssd_voc_cell {                /* 24 bytes, no padding */
    int64_t det_begin, gt_begin;             /* first row of the cell in the packed detection / groundtruth arrays */
    int32_t D, G;                            /* detections, groundtruth boxes                                  */
} ssd_voc_cell;
typedef struct ssd_voc_segment {             /* 24 bytes: the rows of one label in global order                */
    int64_t begin, count, num_gt;
} ssd_voc_segment;
typedef struct ssd_voc_result {              /* 64 bytes */
    double ap, precision, recall, best_threshold, mean_iou;
    int64_t tp, best_index, reserved;        /* reserved: written as 0                                         */
} ssd_voc_result;
int ssd_voc_match(const ssd_voc_cell *cells_host, const ssd_voc_cell *cells_dev, int64_t n_cells,
                  const double *det_box_dev /* [nd,4], cell order */, const int32_t *det_pos_dev /* [nd] */, int64_t nd,
                  const double *gt_box_dev /* [ng,4] */, int64_t ng, double thr,
                  uint8_t *tp_dev /* [n_rows], global order */, double *tp_iou_dev /* [n_rows] */, int64_t n_rows, void *stream);
int ssd_voc_curve(const ssd_voc_segment *segments_host, const ssd_voc_segment *segments_dev, int32_t n_labels,
                  const uint8_t *tp_dev /* [n_rows] */, const double *tp_iou_dev /* [n_rows] */, const double *conf_dev /* [n_rows] */,
                  int64_t n_rows, ssd_voc_result *results_dev /* [n_labels] */, void *stream);

/* ---- tiled detection: frames larger than the network's input as overlapping tiles of the network's own size, one merge NMS ----
 *
 * A frame far larger than min_dimension is served by `ssd_forward` only after shrinking it.  Tiled detection runs the network on
 * overlapping tiles at the frame's own resolution (every tile takes the identity path of the first kernel: no resize, box_scaler 1),
 * optionally on the shrunk whole frame too, and merges all records of a frame with the detector's own NMS rule.  This block is the
 * single statement of the grid and of the merge for the two kernels (csrc/tiles.hip), for tests/helpers/tile_ref.py and for
 * Detector.detect_tiled.
 *
 * The grid of a frame [H, W] under tiles [th, tw] that overlap by oy rows and ox columns (Python: oy = int(overlap * th),
 * ox = int(overlap * tw)):
 *   steps     sy = th - oy,  sx = tw - ox                              (both >= 1)
 *   counts    ny = 1 + ceil((H - th) / sy),  nx = 1 + ceil((W - tw) / sx)
 *   origins   y0(iy) = min(iy * sy, H - th),  x0(ix) = min(ix * sx, W - tw)     (the last tile is pulled back inside the frame)
 *   index     t = (f * ny + iy) * nx + ix   for frame f
 * Origins strictly increase along an axis, the last one is H - th (W - tw), and every pixel lies in a tile.  ssd_tile_grid writes
 * {ny, nx, sy, sx}; both kernels derive the origins from these four numbers, there is no table.  1200 x 1600 under 640 x 640 tiles
 * with oy = ox = 160 gives rows 0, 480, 560 and columns 0, 480, 960; 200 x 301 under 128 x 128 with 32 gives rows 0, 72 and columns
 * 0, 96, 173.
 * Refused (SSD_ERR_INVALID, the reason naming the argument, before any HIP call -- by all three entry points): th or tw that is not a
 * positive multiple of 128; H < th or W < tw (such a frame is ssd_forward's); oy or ox negative; a step below 1; F < 1; a frame
 * block F * H * W * 3 of 2^31 bytes or more (the gather addresses it with 32-bit offsets); more than 2^31 - 1 tiles.
 *
 * ssd_tile_gather: frames_dev uint8 [F, H, W, 3] (any alignment) -> tiles_dev uint8 [F * ny * nx, th, tw, 3], dense, 4-byte
 * aligned; tile t holds rows y0 .. y0 + th - 1, columns x0 .. x0 + tw - 1 of its frame, bit for bit.  One launch on `stream`: no
 * allocation, no synchronisation.  The source is read through a buffer resource of exactly F * H * W * 3 bytes from frames_dev:
 * whole dwords at 4-byte aligned addresses wherever all four bytes lie inside the block, single bytes for the at most two dwords
 * that straddle its ends, so no byte outside the block is ever fetched; a tile row is 3 * tw bytes (a multiple of 384) and is
 * stored as whole 16-byte groups.  Further refusals: a NULL frames_dev / tiles_dev, tiles_dev not 4-byte aligned.
 *
 * ssd_tile_merge: tile_records_dev int32 [F * ny * nx, 6T + 1] (the records of ssd_forward_records on the tiles, T = C * m with
 * C = num_classes, m = max_boxes_per_class) and full_records_dev int32 [F, 6T + 1] (the records of the whole frames; NULL: none)
 * -> out_records_dev int32 [F, 6T + 1], the same layout (boxes [T,4] f32 | scores [T] f32 | labels [T] i32 | num_boxes i32), boxes
 * normalised to the FRAME.
 *   candidates   of (frame f, class c): the rows below num_boxes (clamped to [0, T]) whose label is c, taken from f's tiles in
 *                tile order and then from f's full-frame record, in row order within each source.  The position in this sequence
 *                is the candidate index.  A label outside [0, C) belongs to no class.  Scores are not NaN.
 *   a tile row   moves to frame coordinates one fp32 operation at a time, no contraction, the division correctly rounded:
 *                  Y = ((y * fp32(th)) + fp32(y0)) / fp32(H)  for ymin and ymax,   X = ((x * fp32(tw)) + fp32(x0)) / fp32(W)
 *                its score passes as it is.  A full-frame row passes bit for bit.
 *   selection    tf.image.non_max_suppression's rule as the detector applies it (postprocess.hip, iou_greater): the candidates in
 *                descending score, equal scores by ascending candidate index; a candidate is kept iff iou_greater(candidate, kept,
 *                iou_threshold) is false for every box kept before it; the selection stops at m boxes.  (The comparison is a
 *                strict >, and a box of area <= 0 neither suppresses nor is suppressed.)
 *   output       per frame the classes ascending, within a class the selection order; num_boxes; every row from num_boxes on is
 *                zero.  All 6T + 1 words of every output record are written.
 * Two launches on `stream` (one wave per (frame, class) selects into the output record's own rows c * m ..; one block per frame
 * closes the gaps in place), no allocation, no synchronisation, no atomics: two calls give the same bits.  The candidates of one
 * (frame, class) live in LDS; records from ssd_forward_records hold at most m rows of a class, so there are at most
 * (ny * nx + 1) * m, and a call whose (ny * nx + 1) * m exceeds SSD_TILE_MAX_CANDIDATES is refused before any HIP call (records of
 * another origin with more rows of one class: the candidates past the cap are dropped, never addressed).  Further refusals: NULL
 * tile_records_dev / out_records_dev, a pointer not 4-byte aligned, C < 1, m < 1, C * m above 2^24, a NaN iou_threshold. */
#define SSD_TILE_MAX_CANDIDATES 2048         /* 20 bytes of LDS each: 40 KiB per (frame, class) wave                    */
int ssd_tile_grid(int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy, int32_t ox, int32_t *grid_out /* ny, nx, sy, sx */);
int ssd_tile_gather(const uint8_t *frames_dev /* [F,H,W,3] */, int32_t F, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy,
                    int32_t ox, uint8_t *tiles_dev /* [F*ny*nx,th,tw,3] */, void *stream);
int ssd_tile_merge(const int32_t *tile_records_dev /* [F*ny*nx,6T+1] */, const int32_t *full_records_dev /* [F,6T+1] or NULL */,
                   int32_t F, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy, int32_t ox, int32_t C, int32_t m,
                   float iou_threshold, int32_t *out_records_dev /* [F,6T+1] */, void *stream);

/* ---- the JPEG decoder: baseline JPEG bytes -> uint8 RGB frames in device memory, laid out as ssd_forward_mixed reads them ----
 *
 * Every workload starts from JPEG bytes (inference/evaluate_on_COCO.ipynb reads files, create_tfrecords.py stores them).  The decode
 * splits: parsing and Huffman decoding are serial and run on the HOST (csrc/jpeg_host.cpp, plain C++: ssd_jpeg_info_read,
 * ssd_jpeg_entropy, ssd_jpeg_plan), everything behind the quantised coefficients is integer arithmetic with a fixed definition and
 * runs on the GPU (csrc/jpeg.hip: ssd_jpeg_decode, two launches per batch).  The definition below is the one libjpeg(-turbo)'s
 * default decompressor implements (jidctint.c "slow integer", jdsample.c "fancy" upsampling, jdcolor.c), which is what
 * PIL.Image.open(...).convert("RGB") returns: the frames are that decoder's, bit for bit.  This block is the single statement of
 * the rules for the host stage, for the kernels, for tests/helpers/jpeg_ref.py and for jpeg.py.
 *
 * Accepted streams -- all of:
 *   SOF0 (baseline), sample precision 8, 8-bit quantisation tables (Pq = 0);
 *   ONE scan that interleaves all components (Ns = Nf, the frame's order, Ss = 0, Se = 63, Ah = Al = 0), then EOI;
 *   1 component with sampling 1x1, or 3 components whose chroma factors are 1x1 and whose luma factors (h x v) are 1x1, 2x1 or 2x2;
 *   3 components are YCbCr: a JFIF APP0 was seen; else an Adobe APP14 was seen and its transform is 1; else neither was seen and
 *   the component ids are not 'R', 'G', 'B'.
 *   Restart intervals (DRI + RSTn, numbered modulo 8), optimised Huffman tables, fill bytes FF FF in front of a marker and
 *   APPn / COM segments are handled.
 * SSD_ERR_UNSUPPORTED (the caller decodes the file as before): every other SOFn, DAC, another precision, 16-bit tables, 2 or 4 and
 * more components, other sampling factors (4:4:0, 4:1:1, ..), a scan of fewer components or a second scan, DNL or height 0, RGB or
 * another Adobe transform, and -- from ssd_jpeg_entropy -- a coefficient outside int16 or a stream that is not PINNED (below).
 * SSD_ERR_INVALID: anything malformed or truncated -- no SOI, a segment that runs past the end, an undefined or over-subscribed
 * table, a code that no table holds, a run past coefficient 63, a DC category above 11, entropy data that ends before its last
 * block, a wrong or missing restart marker, no EOI.  The stricter reading is deliberate: such a file goes to the caller's reader.
 *
 * Coefficients: int16 [64] per block in NATURAL (row-major, de-zigzagged) order, NOT dequantised; a component's blocks in raster
 * order over its PADDED block grid, (mcus_y * v) rows by (mcus_x * h) blocks, mcus_x = ceil(width / (8 h_max)), mcus_y =
 * ceil(height / (8 v_max)); the components one after the other.  The DC predictor is kept per component and reset at every restart
 * marker.  Quantisation tables: uint16 [64] in natural order, one per component (components * 64 values).
 *
 * IDCT of a block ("slow integer", CONST_BITS 13, PASS1_BITS 2), on the dequantised values x = coefficient * q:
 *   pass 1 over the COLUMNS of x, every output descaled (t + 2^10) >> 11;
 *   pass 2 over the ROWS of pass 1's result, every output descaled (t + 2^17) >> 18; then + 128, clamped to 0 .. 255.
 *   The order -- columns first, with the intermediate rounding -- is part of the definition.
 *   The one-dimensional kernel on x0 .. x7 (pass 1 takes them as they are, pass 2 likewise; the shifts by 13 are part of it):
 *     even   z1 = (x2 + x6) * 4433,  t2 = z1 - x6 * 15137,  t3 = z1 + x2 * 6270
 *            t0 = (x0 + x4) << 13,  t1 = (x0 - x4) << 13
 *            t10 = t0 + t3,  t13 = t0 - t3,  t11 = t1 + t2,  t12 = t1 - t2
 *     odd    a = x7, b = x5, c = x3, d = x1
 *            z1 = a + d,  z2 = b + c,  z3 = a + c,  z4 = b + d,  z5 = (z3 + z4) * 9633
 *            a *= 2446,  b *= 16819,  c *= 25172,  d *= 12299
 *            z1 *= -7373,  z2 *= -20995,  z3 = z3 * -16069 + z5,  z4 = z4 * -3196 + z5
 *            a += z1 + z3,  b += z2 + z4,  c += z2 + z3,  d += z1 + z4
 *     out    0 .. 7 = t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d
 *   (0.298631336 = 2446, 0.390180644 = 3196, 0.541196100 = 4433, 0.765366865 = 6270, 0.899976223 = 7373, 1.175875602 = 9633,
 *    1.501321110 = 12299, 1.847759065 = 15137, 1.961570560 = 16069, 2.053119869 = 16819, 2.562915447 = 20995, 3.072711026 = 25172.)
 *   All arithmetic is 32-bit two's complement (the code forms the sums in uint32), all right shifts are arithmetic.
 *   This wrap-and-clamp definition is what the kernels compute on ANY coefficients and tables (tests/test_gpu_jpeg.py holds them to
 *   it over all of int16 x uint16); it is the library's result only for pinned streams.
 *
 * Pinned streams.  With x, w (pass 1's descaled outputs) and v (pass 2's descaled outputs, before + 128) taken as EXACT integers,
 * nothing wrapped, a stream is pinned if and only if in every block of every component
 *     every |x| <= 16383,   every |w| <= 16383,   every v in [-512, 511].
 *   Why these: with inputs of at most 16383 no sum of the one-dimensional kernel leaves int32 in either pass (the largest, t10 + d,
 *   stays below 61214 * 16383 ~ 1.0e9), so the 32-bit wrap above, the library's C path and its SIMD paths form the same numbers;
 *   the SIMD paths' 16-bit pair sums (x0 +- x4, x1 + x5, ..) fit int16 and a saturating 16-bit workspace never saturates; and for
 *   v in [-512, 511] every path's clamp -- a range table indexed by (v + 128) & 1023, or a saturating pack -- is the plain clamp
 *   to 0 .. 255.  Outside, the library's own paths stop agreeing with each other (a table that wraps at 1024 against a pack that
 *   saturates, 16-bit sums that wrap or saturate), so "what PIL returns" depends on the build and the CPU, and nothing can be
 *   pinned: with the earlier rule |coefficient * q| <= 32767, files under loud constant tables gave frames up to 255 counts from
 *   PIL's from |coefficient * q| = 2920 on.  The v limb binds first: |w| > 16383 or |x| > 16383 in a block imply
 *   some |v| of about 512 and 2048 there.  Files encoded from pixels stay a factor 2 to 4 inside every limb.
 *   ssd_jpeg_entropy tests the rule block by block: S = sum |x| <= 2047 implies all three limbs (the derivation stands in
 *   csrc/jpeg_host.cpp), and a louder block goes through both passes in 64-bit integers on the host.
 *
 * Upsampling of a chroma plane s with REAL extents n = ceil(width / 2) columns and, for 2x2, m = ceil(height / 2) rows (samples
 * outside the real extent are never read: block padding is no neighbour, edges replicate the last real sample):
 *   2x1   per row:  out[2i] = (3 s[i] + s[i-1] + 1) >> 2,  out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2;  out[0] = s[0], out[2n-1] = s[n-1]
 *   2x2   output row 2j + v: the neighbour row nb = j - 1 for v = 0, j + 1 for v = 1 (row -1 is row 0, row m is row m - 1);
 *         c[i] = 3 s[j][i] + s[nb][i];  out[2i] = (3 c[i] + c[i-1] + 8) >> 4,  out[2i+1] = (3 c[i] + c[i+1] + 7) >> 4;
 *         out[0] = (4 c[0] + 8) >> 4,  out[2n-1] = (4 c[n-1] + 7) >> 4
 *   n <= 2 (width <= 4): both modes REPLICATE each sample (2x1 or 2x2) instead -- the library's rule.
 *   The result is cropped to height x width.
 * Colour, with cb, cr centred by -128:
 *   R = Y + ((91881 cr + 32768) >> 16),  B = Y + ((116130 cb + 32768) >> 16),  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)
 *   (one arithmetic shift of the signed sum), each clamped to 0 .. 255.  One component: R = G = B = Y.
 *
 * Host stage (no HIP, no global state, re-entrant; never reads outside [bytes, bytes + n), never writes outside what `info` reports):
 *   ssd_jpeg_info_read  parses the whole marker structure (headers, the scan's extent up to EOI) and fills *out.
 *   ssd_jpeg_entropy    decodes the scan into coef_host [info->coef_count] and quant_host [info->components * 64]; `info` must be
 *                       what ssd_jpeg_info_read gave for these bytes (SSD_ERR_INVALID otherwise); SSD_ERR_UNSUPPORTED for a
 *                       stream that is not pinned, from the first block outside the rule.  After a refusal the two
 *                       arrays hold unspecified values inside their bounds.
 *   ssd_jpeg_plan       the batch layout: images_out[b] for infos[b], b < B, in order -- coefficients back to back (64 * blocks
 *                       each), tables back to back, each image's sample planes on the next 16-byte boundary of the workspace,
 *                       each frame on the next 16-byte boundary (ssd_forward_mixed's default layout), block_begin / tile_begin the
 *                       running sums -- and totals_out = {coefficients (int16), table values (uint16), workspace bytes, frame
 *                       bytes}.  SSD_ERR_INVALID for an info no accepted stream gives, or frames of 2^31 bytes and more.
 * Device stage: ssd_jpeg_decode enqueues two launches on `stream` whatever B and the sizes are; no allocation, no synchronisation,
 * no atomics, no handle; every byte of every frame is written exactly once, no byte between frames, two calls give the same bytes.
 *   images_host / images_dev  the same B rows in host memory (read by the call, which refuses a bad table before any HIP call) and in
 *                       device memory (8-byte aligned; the kernels read it; the caller's upload, ordered before the call on `stream`)
 *   coef_dev, quant_dev 16-byte aligned; an image's coefficients at coef_offset (a multiple of 8), its tables at quant_offset (a
 *                       multiple of 8)
 *   workspace_dev       16-byte aligned, ssd_jpeg_workspace_bytes(images_host, B) bytes: the sample planes of component k of an
 *                       image, pitch 8 * blocks per row, at plane_offset (a multiple of 8) + 64 * the blocks of the components before
 *   frames_dev          16-byte aligned; frame b = uint8 [height, width, 3] at frame_offset (a multiple of 16), within 2 GiB
 *   launch 1            dequantise + IDCT: 8 lanes per block, a wave reads 8 blocks as 1 KiB of 16-byte row loads; 32 blocks per
 *                       256-lane group, at most SSD_COCO_GRID_CAP groups striding over all blocks of the batch
 *   launch 2            upsample + convert + crop: a 256-lane group takes a tile of SSD_JPEG_TILE consecutive pixels (row-major) of
 *                       ONE frame, so the sampling mode is uniform in the group; a lane owns a run of SSD_JPEG_RUN of them (48
 *                       bytes: three 16-byte stores; a frame's last, shorter run stores its bytes singly); at most
 *                       SSD_COCO_GRID_CAP groups striding over all tiles of the batch
 *   Refused with SSD_ERR_INVALID, the reason "ssd_jpeg_decode: ..." naming the argument: B outside [0, 2^20]; NULL or misaligned
 *   pointers with B > 0; a row whose geometry no accepted stream gives; offsets that are negative, misaligned, or not ascending and
 *   disjoint (planes, frames); block_begin / tile_begin that are not the running sums; a frame that ends past 2^31 - 1.  B == 0
 *   enqueues nothing. */
#define SSD_JPEG_RUN 16                      /* pixels a lane of launch 2 owns                                          */
#define SSD_JPEG_TILE 4096                   /* pixels a 256-lane group of launch 2 takes: 256 runs                     */
typedef struct ssd_jpeg_info {               /* 56 bytes, no padding */
    int32_t height, width, components;       /* 1 or 3 components                                               */
    int32_t h, v;                            /* luma sampling factors: 1x1, 2x1 (4:2:2) or 2x2 (4:2:0)         */
    int32_t mcus_x, mcus_y, restart_interval;    /* restart_interval in MCUs, 0: none                          */
    int32_t blocks[3];                       /* blocks of each component (0 for an absent one)                 */
    int32_t reserved;                        /* 0                                                              */
    int64_t coef_count;                      /* 64 * (blocks[0] + blocks[1] + blocks[2])                       */
} ssd_jpeg_info;
typedef struct ssd_jpeg_image {              /* 80 bytes, no padding: one image of a batch                     */
    int32_t height, width, components, h, v, mcus_x, mcus_y, reserved;
    int64_t coef_offset;                     /* int16 elements from coef_dev                                   */
    int64_t quant_offset;                    /* uint16 elements from quant_dev                                 */
    int64_t plane_offset;                    /* bytes from workspace_dev                                       */
    int64_t frame_offset;                    /* bytes from frames_dev                                          */
    int64_t block_begin;                     /* blocks of the images before this one                           */
    int64_t tile_begin;                      /* tiles (ceil(height * width / SSD_JPEG_TILE)) of the images before */
} ssd_jpeg_image;
int ssd_jpeg_info_read(const uint8_t *bytes, int64_t n, ssd_jpeg_info *out);
int ssd_jpeg_entropy(const uint8_t *bytes, int64_t n, const ssd_jpeg_info *info, int16_t *coef_host, uint16_t *quant_host);
int ssd_jpeg_plan(const ssd_jpeg_info *infos, int32_t B, ssd_jpeg_image *images_out, int64_t *totals_out /* [4] */);
size_t ssd_jpeg_workspace_bytes(const ssd_jpeg_image *images_host, int32_t B);     /* 0 for a table ssd_jpeg_decode refuses */
int ssd_jpeg_decode(const ssd_jpeg_image *images_host, const ssd_jpeg_image *images_dev, int32_t B, const int16_t *coef_dev,
                    const uint16_t *quant_dev, void *workspace_dev, uint8_t *frames_dev, void *stream);

/* ---- the JPEG encoder: uint8 RGB frames in device memory -> baseline JPEG bytes, the write-side twin of the block above ----
 *
 * data/create_tfrecords.py re-encodes every grayscale file as an RGB JPEG with PIL's default save (to_jpeg_bytes); python -m
 * ssd_amd.create_tfrecords --jpeg_device does the same without a pixel on the host.  The encode splits where the decode does:
 * everything in front of the quantised coefficients is integer arithmetic with a fixed definition and runs on the GPU
 * (csrc/jpeg_enc.hip: ssd_jpeg_encode, two launches per batch), the Huffman coding and the marker structure are serial and run
 * on the HOST (csrc/jpeg_emit.cpp, plain C++: ssd_jpeg_emit).  The definition below is the one libjpeg(-turbo)'s default
 * compressor implements (jccolor.c, jcsample.c, jfdctint.c "slow integer", jcdctmgr.c, jchuff.c, jcmarker.c -- public algorithms,
 * restated), which is what PIL's Image.save(format="jpeg") writes: the files are that encoder's, byte for byte.  This block is the
 * single statement of the rules for the kernels, the host stage, tests/helpers/jpeg_enc_ref.py and jpeg.py.
 *
 * Input: uint8 RGB frames [height, width, 3], height and width from 1 to 65 535; any byte address.
 * quality 1 .. 100 (PIL's default: 75) by jpeg_quality_scaling: scale = 5000 / quality (integer division) below 50, else
 *   200 - 2 quality; entry = clamp((base * scale + 50) / 100, 1, 255) on the Annex K base tables (luma for component 0, chroma for
 *   components 1 and 2).  ssd_jpeg_quant_tables writes the two tables, uint16 [2][64] in natural order.
 * sampling: SSD_JPEG_SAMPLING_420 (luma 2x2, PIL's default) or SSD_JPEG_SAMPLING_444 (1x1); chroma factors are 1x1.  Any other
 *   value, 422 included, is SSD_ERR_UNSUPPORTED.  Anything else out of range is SSD_ERR_INVALID.
 *
 * Colour (16 fractional bits; every sum is positive and below 2^32, the code forms it in uint32):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 * Geometry as the decoder's: mcus_x = ceil(width / (8 h)), mcus_y = ceil(height / (8 v)); a component's PADDED grid is
 *   (mcus_y * v_c) rows by (mcus_x * h_c) blocks.  Its OWN whole blocks are ceil(width h_c / (8 h)) by ceil(height v_c / (8 v)).
 * Edge replication: a full-size plane (luma; chroma of 4:4:4) continues its last column and its last row.
 * Downsampling (4:2:0 chroma, "h2v2" box): the converted plane continues its last column first, and its last row to an even row
 *   count; out[j][i] = (s[2j][2i] + s[2j][2i+1] + s[2j+1][2i] + s[2j+1][2i+1] + bias) >> 2 with bias 1 for even i, 2 for odd i
 *   (every output column counts, replicated ones too); the ceil(height / 2) rows so formed then continue their last ROW.
 * Forward DCT of a block ("slow integer", CONST_BITS 13, PASS1_BITS 2) on d = sample - 128:
 *   pass 1 over the ROWS, pass 2 over the COLUMNS of pass 1's result; D(x, n) = (x + 2^(n-1)) >> n, arithmetic shift.
 *   The one-dimensional kernel on d0 .. d7, n = 11 in pass 1 and 15 in pass 2:
 *     t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *     t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *     out0, out4 = (t10 + t11) << 2, (t10 - t11) << 2 in pass 1;  D(t10 + t11, 2), D(t10 - t11, 2) in pass 2
 *     z1 = (t12 + t13) * 4433;  out2 = D(z1 + t13 * 6270, n),  out6 = D(z1 - t12 * 15137, n)
 *     z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633
 *     t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299
 *     z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5
 *     out7 = D(t4 + z1 + z3, n), out5 = D(t5 + z2 + z4, n), out3 = D(t6 + z2 + z3, n), out1 = D(t7 + z1 + z4, n)
 *   32-bit two's complement (the code forms the sums in uint32: nothing rests on signed overflow; no sum leaves int32 here).
 * Quantisation: the result carries a factor 8; coefficient = sign(x) * ((|x| + 4 q) / (8 q)), integer division: x / (8 q)
 *   rounded to nearest, halves away from zero.
 * Dummy blocks: a component's plane is replicated only up to its OWN whole blocks; the remaining blocks of its padded grid (4:2:0
 *   luma with an odd count of 8-blocks in either direction) are dummy blocks: all AC coefficients zero, the DC of the block coded
 *   before it.  In the stream a dummy block is therefore "DC difference 0, end of block", and the predictor is unchanged.
 * Coefficients: THE DECODER'S LAYOUT -- int16 [64] per block in natural order, quantised, a component's blocks in raster order
 *   over its padded grid, the components one after the other.  ssd_jpeg_encode writes dummy blocks as 64 zeros; ssd_jpeg_emit
 *   never reads them.
 * The file, in this order: SOI; APP0 JFIF 1.01, units 0, density 1 x 1, no thumbnail; DQT table 0; DQT table 1 (8-bit entries in
 *   zigzag order); SOF0 (precision 8; components 1, 2, 3 with tables 0, 1, 1); DHT DC 0, AC 0, DC 1, AC 1: the Annex K tables, not
 *   optimised; SOS (tables 0/0, 1/1, 1/1; 0, 63, 0); the scan; EOI.  No restart interval.  The scan: MCUs in raster order, in an
 *   MCU the luma blocks (row by row) then Cb then Cr; per block the DC difference to the component's predictor as category +
 *   bits, the AC coefficients in zigzag order as (run, category) + bits with ZRL (F0) for 16 zeros and EOB (00) behind the last
 *   non-zero one; a negative value v is coded as the low bits of v - 1; FF in the data is followed by 00; the last byte is
 *   filled with 1-bits.
 *
 * Host stage (csrc/jpeg_emit.cpp: no HIP, no global state beyond constant tables, re-entrant, no thread pool: the callers' threads
 * run images in parallel):
 *   ssd_jpeg_quant_tables  the two tables of `quality`.
 *   ssd_jpeg_emit_bound    a size no file of this geometry exceeds (1024 + 416 per block of the padded grids), or the refusal (< 0).
 *   ssd_jpeg_emit          writes the whole file of ONE image from its coefficients (coef: the image's first coefficient, the
 *                          layout above) into out[0, capacity) and its size into *size_out.  A capacity below the file's size is
 *                          SSD_ERR_INVALID; nothing is ever written at or past out + capacity.  After a refusal out holds
 *                          unspecified bytes inside its capacity.  NULL coef / out (with capacity > 0) / size_out: SSD_ERR_INVALID.
 *   ssd_jpeg_encode_plan   the batch layout, as ssd_jpeg_plan: images_out[b] for frames[b] = {height, width, sampling, quality},
 *                          in order (a batch may mix samplings and qualities) -- frames on 16-byte boundaries one after the
 *                          other (ssd_jpeg_plan's layout of them), each image's
 *                          sample planes on the next 16-byte boundary of the workspace, coefficients back to back (128 bytes per
 *                          block: 16-byte boundaries), block_begin / tile_begin the running sums -- and totals_out = {coefficients
 *                          (int16), workspace bytes, frame bytes, blocks}.
 * Device stage: ssd_jpeg_encode enqueues two launches on `stream` whatever B and the sizes are; no allocation, no synchronisation,
 * no atomics, no handle; two calls give the same bytes.
 *   images_host / images_dev  the same B rows in host memory (checked by the call before any HIP call) and in device memory (8-byte
 *                       aligned; the kernels read it); a row carries its own sampling (h, v) and quality
 *   frames_dev          frame b = uint8 [height, width, 3] at frame_offset (any byte offset >= 0)
 *   workspace_dev       16-byte aligned, ssd_jpeg_encode_workspace_bytes(images_host, B) bytes: component k's padded sample plane,
 *                       pitch 8 * blocks per row, at plane_offset (a multiple of 16) + 64 * the blocks of the components before
 *   coef_dev            16-byte aligned; an image's coefficients at coef_offset (a multiple of 8), 64 * blocks of them
 *   launch 1            convert + replicate + downsample: a 256-lane group takes a tile of SSD_JPEG_ENC_TILE units of ONE image, so
 *                       the sampling is uniform in the group; a unit is 8 chroma samples of one row of the padded chroma plane
 *                       with the 8 h by v luma samples they cover (one lane: 8-byte chroma stores, 8 h-byte luma stores).  Every
 *                       sample of the padded planes is written (those of dummy blocks hold replicated values nobody reads).
 *   launch 2            level shift + both DCT passes + quantise: 8 lanes per block, 32 blocks per 256-lane group, the block's tile
 *                       in LDS; lane r scales row r of the base table by the image's quality and stores row r of the block as
 *                       ONE 16-byte store.  Every coefficient of every padded grid is
 *                       written exactly once, dummy blocks as zeros; no byte between two images' coefficients is written.
 *   Both launches: at most SSD_COCO_GRID_CAP groups striding over the batch's tiles / blocks.
 *   Refused before any HIP call: SSD_ERR_UNSUPPORTED for a row whose (h, v) is neither 1x1 nor 2x2; SSD_ERR_INVALID, the reason
 *   "ssd_jpeg_encode: ..." naming the argument, for B outside [0, 2^20], a row's quality outside 1 .. 100, NULL or misaligned pointers
 *   with B > 0, a row whose height, width or MCU counts are not the geometry above, offsets that are negative or misaligned,
 *   planes or coefficients that do not ascend disjointly, block_begin / tile_begin that are not the running sums.  B == 0
 *   enqueues nothing. */
#define SSD_JPEG_SAMPLING_444 444
#define SSD_JPEG_SAMPLING_420 420
#define SSD_JPEG_ENC_TILE 256                /* units a 256-lane group of launch 1 takes: one per lane                  */
typedef struct ssd_jpeg_encode_image {       /* 72 bytes, no padding: one image of a batch                     */
    int32_t height, width, h, v, mcus_x, mcus_y, quality, reserved;
    int64_t frame_offset;                    /* bytes from frames_dev                                          */
    int64_t plane_offset;                    /* bytes from workspace_dev                                       */
    int64_t coef_offset;                     /* int16 elements from coef_dev                                   */
    int64_t block_begin;                     /* blocks of the images before this one                           */
    int64_t tile_begin;                      /* tiles (ceil(8 * mcus_y * mcus_x / SSD_JPEG_ENC_TILE)) of the images before */
} ssd_jpeg_encode_image;
int ssd_jpeg_quant_tables(int32_t quality, uint16_t *tables_out /* [2][64] */);
int64_t ssd_jpeg_emit_bound(int32_t height, int32_t width, int32_t sampling);
int ssd_jpeg_emit(const int16_t *coef, int32_t height, int32_t width, int32_t sampling, int32_t quality, uint8_t *out,
                  int64_t capacity, int64_t *size_out);
int ssd_jpeg_encode_plan(const int32_t *frames /* [B][4] */, int32_t B, ssd_jpeg_encode_image *images_out, int64_t *totals_out /* [4] */);
size_t ssd_jpeg_encode_workspace_bytes(const ssd_jpeg_encode_image *images_host, int32_t B);   /* 0 for a table ssd_jpeg_encode refuses */
int ssd_jpeg_encode(const ssd_jpeg_encode_image *images_host, const ssd_jpeg_encode_image *images_dev, int32_t B,
                    const uint8_t *frames_dev, void *workspace_dev, int16_t *coef_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_H */
