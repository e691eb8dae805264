/*
 * yolonano_hip.h — C ABI of libyolonano_hip.so, the MI355X (gfx950) YOLO-Nano hot path.
 *
 * The reference (yjh0410/YOLO-Nano) has no FFI/plugin interface: its boundary is the Python
 * surface of `YOLONano` (models/yolo_nano.py:12-376).  This header is the C boundary that sits
 * directly under that surface; every entry point names the reference code it replaces.  The host
 * shim `yolo_nano_amd.YOLONano` binds these with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every function returns 0 on success, non-zero on failure; yn_last_error(h) gives the text
 *     (yn_last_error(NULL) for a failed yn_create).
 *   - one handle = one device + one HIP stream; a handle is not thread-safe.
 *   - "dev" pointers are device (HBM) pointers owned by the caller; the handle owns only its
 *     weights and its activation workspace.  Nothing here synchronises the stream unless noted.
 *   - activations cross this boundary as float32.  Raw head tensors are NHWC
 *     [B, H, W, A*(1+C+4)] — the layout models/yolo_nano.py:312 permutes to before splitting.
 *   - candidate index  n = off_s + (y*W_s + x)*A + a ,  scales in order stride 8, 16, 32
 *     (models/yolo_nano.py:308-330);  N = A * sum_s (S/stride_s)^2.
 */
#ifndef YOLONANO_HIP_H
#define YOLONANO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yn_handle yn_handle;

enum { YN_BACKBONE_0_5X = 0, YN_BACKBONE_1_0X = 1, YN_BACKBONE_1_5X = 2, YN_BACKBONE_2_0X = 3 };
enum { YN_ACT_NONE = 0, YN_ACT_RELU = 1, YN_ACT_LEAKY = 2 };
enum { YN_F32 = 0, YN_F16 = 1 };
/* return values: 0 = success, 1 = failure (yn_last_error has the text), YN_STATUS_RANGE = yn_infer / yn_pack_detections refused because an EARLIER
 * yn_infer on this handle left the split-f16 range and nobody has acknowledged it through yn_range_status yet (see there) */
enum { YN_STATUS_OK = 0, YN_STATUS_ERROR = 1, YN_STATUS_RANGE = 2 };

/* Mirrors YOLONano.__init__(device, input_size, num_classes, trainable, conf_thresh, nms_thresh,
 * anchor_size, backbone, diou_nms)  — models/yolo_nano.py:13-27. */
typedef struct yn_config {
    int   input_size;      /* S, multiple of 32 */
    int   num_classes;     /* C */
    int   num_anchors;     /* A per scale (3) */
    float anchors[18];     /* [3 scales][A][w,h] in input pixels (data/config.py:11-17) */
    int   backbone;        /* YN_BACKBONE_* (backbone/shufflenetv2.py:95-102) */
    float conf_thresh;     /* models/yolo_nano.py:19 */
    float nms_thresh;      /* models/yolo_nano.py:20 */
    int   diou_nms;        /* models/yolo_nano.py:21 */
    int   max_batch;       /* workspace is sized for this many images at input_size */
    int   device;          /* HIP device ordinal */
    void* stream;          /* hipStream_t; NULL = default stream */
} yn_config;

/* ---- lifetime / configuration -------------------------------------------------------------- */
int  yn_abi_version(void);
int  yn_create(const yn_config* cfg, yn_handle** out);          /* YOLONano.__init__            :13  */
void yn_destroy(yn_handle* h);
const char* yn_last_error(yn_handle* h);
/* device memory the library holds in this process, over every handle and object: blocks and bytes (either pointer may be NULL).  A card's free
 * memory is shared with other processes and cannot show that a destroy gave everything back; this count can. */
int  yn_live_device_memory(int64_t* blocks, int64_t* bytes);
int  yn_set_grid(yn_handle* h, int input_size);                 /* YOLONano.set_grid            :115 */
/* Rectangular inference.  A rectangular grid is a WINDOW OF A LETTERBOXED SQUARE: the canvas is height x width (positive multiples of 32),
 * its top-left pixel sits at (left, top) of a side x side square, 0 <= left, left + width <= side, 0 <= top, top + height <= side.
 *   input        x_dev [B][3][height][width]
 *   raw heads    NHWC [B][height/8][width/8][A(5+C)], then /16, /32;  N = A * sum_s (height/st_s)(width/st_s)
 *   candidates   scale first, then cell gy * (width/st) + gx, then anchor
 *   boxes        normalised to the SQUARE, not the canvas: with p the canvas pixel coordinate, v = (p + off) / (float)side clamped to [0, 1],
 *                off = left for x1 / x2, top for y1 / y2 - one normaliser for both axes.  So every consumer of the packed records
 *                (yn_pack_detections -> yn_eval_add, yn_coco_add, yn_draw_batch) keeps the ordinary 7-field letterbox geometry of the square.
 * A 1280x720 frame letterboxed to 640 is 640x360 of picture between two 140-row bands of pad; the 640x384 window at (0, 128) holds it all
 * in 0.6 of the pixels.  The run differs from the square one only through what the convs see at the cut (zero padding instead of the pad's
 * activations).  side = 0: side = max(height, width), the window centred (left / top are ignored).  The window that IS the whole square
 * (height == width == side, left == top == 0) is yn_set_grid(side): the same code path, the same bits.
 * Follow the grid: yn_forward_raw, yn_forward_taps, yn_score_full, yn_decode_boxes (canvas pixels, no offset), yn_infer, yn_postprocess,
 * yn_pack_detections, yn_op_decode_cand, yn_op_head_tail.  Refused on a window grid ("... needs a square grid", nothing launched, the grid
 * unchanged): yn_train_step, yn_train_forward, yn_loss, yn_loss_heads, yn_op_h16_loss, yn_make_targets, yn_tta_infer, yn_slice_append,
 * yn_slice_infer. */
int  yn_set_grid_rect(yn_handle* h, int height, int width, int side, int left, int top);
int  yn_grid_shape(yn_handle* h, int* height, int* width, int* side, int* left, int* top);   /* any pointer may be NULL */
int  yn_set_stream(yn_handle* h, void* stream);                /* drains the previous stream first  */
int  yn_set_thresholds(yn_handle* h, float conf_thresh, float nms_thresh, int diou_nms);
int  yn_num_predictions(yn_handle* h);                          /* N for the current grid            */
int  yn_use_graph(yn_handle* h, int enable);                    /* hipGraph-capture yn_infer/forward */
int  yn_synchronize(yn_handle* h);
/* Inside one forward the executor forks independent kernel chains (the two branches of a stride-2 unit, the laterals, the heads)
 * onto two side streams of the handle (default on: +4 % for a single handle).  A caller that already runs several handles
 * concurrently on its own streams should turn it off — nine streams contending cost 10 % at three handles (24.1 k vs 21.7 k images/s). */
int  yn_multi_stream(yn_handle* h, int enable);
/* The MFMA-bound convolutions (the dense 3x3 neck layers) run on the f16 matrix pipe with SPLIT fp32 operands by default —
 * x = hi + lo*2^-11, three f16 MFMAs per product into fp32 accumulators: fp32-class results (per-product error <= ~3*2^-22; the
 * f32 MFMA of gfx950 runs at 1/16 of the f16 rate and there is no TF32).  enable != 0 pins every conv to the f32 MFMA. */
int  yn_exact_f32(yn_handle* h, int enable);
/* RANGE of the split-f16 family, and its guard.  hi = (f16)x is finite only for |x| < 65520, so the default path needs every folded
 * GEMM weight and every activation that enters a GEMM-shaped conv below 65504 (normalised inputs, BatchNorm-folded weights and the
 * activations they produce are O(1)..O(100); the reference's fp32 has no such limit).  Checked, not assumed:
 *   - weights: yn_fold_bn tests every folded pointwise / dense-3x3 weight on the device; if one is >= 65504 (or not finite) the handle
 *     runs the f32-MFMA family from then on, exactly as under yn_exact_f32(1)  (*weights_exceed_f16 = 1);
 *   - activations: every kernel that splits activations tracks the largest |x| it split and raises a flag in HBM when it reached
 *     65504; *activation_overflow returns that flag for everything issued since the last call and clears it.  The call synchronises
 *     the handle's stream.  A set flag means the results of those calls are NOT valid: re-run them after yn_exact_f32(h, 1)
 *     (the host shim yolo_nano_amd.YOLONano does this by itself, once, and stays on the f32-MFMA family).
 *     yn_infer also delivers the flag WITH its results, at no extra synchronisation: while it is set every count_dev[b] comes back
 *     NEGATIVE (-1 - K_b), and yn_pack_detections carries the mark on as offsets_dev[B] = -1 - total.  The flag is sticky until
 *     yn_range_status clears it.  The same fact OUT OF BAND, for callers that loop `i < count[b]` without looking at the sign: the kernel
 *     that writes the negative counts also sets one word of pinned host memory, and from then on every yn_infer / yn_pack_detections
 *     on the handle returns YN_STATUS_RANGE (checked on the host, no synchronisation) until yn_range_status has been called - or
 *     yn_exact_f32(h, 1) is in force (the f32-MFMA family cannot leave the range: running again under it is the recovery).  The out-of-band
 *     check is BEST EFFORT for pipelined calls: a yn_infer enqueued before the marking kernel has run is not refused; the negative counts
 *     always travel with the results themselves.
 *     yn_range_status also reports (return 1 + yn_last_error) an expired bounded wait of stage_pipe_kernel (yn_stage_fuse).
 * Tiny values need no guard: below the f16 normal range lo = (x - hi) * 2^11 still carries x. */
int  yn_range_status(yn_handle* h, int* weights_exceed_f16, int* activation_overflow);
/* yn_infer only: the last pointwise conv of each detection head (models/yolo_nano.py:299-301) and the decode of that scale's
 * candidates (:308-330, 362-367) run as ONE kernel, so the raw head tensors are neither written nor re-read (default on; needs
 * the split-f16 family and A(5+C) <= 256, otherwise yn_infer runs head GEMM + decode kernel as before).  Outputs are bit-identical
 * either way: a speed switch for A/B runs.  enable = 1: when the stride-8 head has >= 8192 pixels (below that three GEMMs + one decode
 * launch are faster), 2: always. */
int  yn_fuse_decode(yn_handle* h, int enable);
/* Layer k of the three detection heads (models/yolo_nano.py:299-301: same operator, three pyramid levels) and the three FPN
 * laterals (:286-288) run as ONE grouped launch each instead of three (default on; split-f16 family only).  Bit-identical outputs:
 * a speed switch for A/B runs. */
int  yn_group_launch(yn_handle* h, int enable);
/* A stride-2 ShuffleV2 unit (backbone/shufflenetv2.py:30-51, 73-74: branch 2 = pointwise -> depthwise stride 2 -> pointwise, branch 1 =
 * depthwise stride 2 -> pointwise, then concat + channel shuffle) as ONE kernel for the widths it is built for (24 input channels,
 * branch width 58 or 24: stage 2 of 1.0x / 0.5x, whose intermediate is the largest tensor of the network); the wider units (stages 3 / 4, branch width <= 256) as
 * their first pointwise conv + ONE kernel for everything behind it.  Default on, split-f16 family only, bit-identical to the five
 * launches. */
int  yn_down_fuse(yn_handle* h, int enable);
/* Layers .2 + .3 + .4 of the three detection heads and the candidate decode as ONE grouped kernel — depthwise 3x3 + pointwise conv +
 * last conv + decode on an 8 x 4 pixel tile; layer .3's activation never reaches memory (models/yolo_nano.py:60-82, 299-330, 362-367).
 * Default on; needs yn_fuse_decode and yn_group_launch in effect and a head of 129..256 columns (COCO); otherwise, or with 0, two
 * grouped kernels (depthwise + pointwise, last conv + decode).  Bit-identical either way. */
int  yn_tail_fuse(yn_handle* h, int enable);
/* Per-class NMS (models/yolo_nano.py:159-188, 263-272): resolve the 64 best-scored boxes of every class first and drop every later box
 * one of their KEPT boxes suppresses before the dense pairwise phase (exact: a removed box suppresses nothing).  mode 0 = off, 1 (default) =
 * for batches of >= 4 images, 2 = always.  Same kept sets either way. */
int  yn_nms_prefilter(yn_handle* h, int mode);
/* Large class segments (> 1 024 boxes behind the prefilter) whose boxes are spread out get their suppression words from a sweep over bins of
 * the boxes' left edges - only pairs whose x-extents intersect are evaluated, with the same exact predicate (models/yolo_nano.py:159-188: `ovr <=
 * thresh` keeps) - instead of the dense 64 x 64 tiles; the kernel decides per segment from a pair-count estimate.  1 (default) / 0: every segment
 * dense.  Kept sets are identical either way. */
int  yn_nms_sweep(yn_handle* h, int enable);
/* Testing aid: how many (image, class) segments of the LAST yn_infer / yn_postprocess call (B images, C classes) the sweep handled
 * (synchronises the handle's stream); -1 on a failed copy. */
int  yn_nms_sweep_segments(yn_handle* h, int B, int C);
/* Testing aid: the state the per-class NMS chain of the LAST yn_postprocess / yn_infer / yn_nms_merge call (B images, N candidates, C
 * classes: they must be that call's, else an error) left in the handle's scratch, copied to HOST buffers (synchronises the handle's
 * stream; any pointer may be NULL).  A normal call pays nothing for it: the plan is a host-side record of the decisions the launch function
 * took anyway, everything else already sits in the scratch.  (A yn_infer that replays a captured graph launches nothing on the host: the
 * plan is then the one recorded at the last capture or eager call - turn yn_use_graph off to inspect a yn_infer.)
 *   plan[YN_NMS_PLAN_INTS]  the launch plan, indexed by YN_NMS_PLAN_*: which kernels ran (few-segments route, fused bucket + sort, chunked
 *                           sort, merge, prefilter with its sliced ranks, sweep with its LDS form / slots / workgroups per segment, resolve
 *                           as one launch or split, DIoU)
 *   seg_count, seg_off [B][C]   boxes per class and the class's first position
 *   bucket [B][N], sbox [B][N][4]   per class at seg_off: candidate ids by (score descending, id descending) and their boxes
 *   seg_count2 [B][C], bucket2 [B][N], sbox2 [B][N][4], seg_sparse [B][C]   only where plan[YN_NMS_PLAN_PREFILTER] is set (else left
 *                           untouched): the prefilter's survivors per class at seg_off, and 1 for the classes handed to the sweep
 *   keep [B][N]             the kept flags by candidate id (what compact_kernel read) */
#define YN_NMS_PLAN_B             0
#define YN_NMS_PLAN_N             1
#define YN_NMS_PLAN_C             2
#define YN_NMS_PLAN_FEW           3
#define YN_NMS_PLAN_FUSED         4
#define YN_NMS_PLAN_CHUNKS        5
#define YN_NMS_PLAN_MERGE         6
#define YN_NMS_PLAN_PREFILTER     7
#define YN_NMS_PLAN_PRE_RANKS     8
#define YN_NMS_PLAN_SWEEP         9
#define YN_NMS_PLAN_SWEEP_MAXN    10
#define YN_NMS_PLAN_SWEEP_SLOTS   11
#define YN_NMS_PLAN_SWEEP_SPLIT   12
#define YN_NMS_PLAN_RESOLVE_ONE   13
#define YN_NMS_PLAN_RESOLVE_SPLIT 14
#define YN_NMS_PLAN_DIOU          15
#define YN_NMS_PLAN_INTS          16
int  yn_nms_stages(yn_handle* h, int B, int N, int C, int32_t* plan, int32_t* seg_count, int32_t* seg_off, int32_t* bucket, float* sbox,
                   int32_t* seg_count2, int32_t* bucket2, float* sbox2, int32_t* seg_sparse, int32_t* keep);
/* Per-layer tile autotuning of the pointwise-conv GEMM (default on): the first eager execution of a layer
 * shape times every instantiated tile configuration of the layer's family (split-f16 by default, f32-MFMA under yn_exact_f32) on
 * the handle's stream and caches the fastest.  All configurations of a family produce bit-identical results; disabling falls back
 * to a static heuristic. */
int  yn_autotune(yn_handle* h, int enable);
/* Testing aid: pin every pointwise GEMM of this handle to tile configuration `index` (0 <= index < yn_pw_config_count();
 * a configuration that does not cover a layer's strides falls back to the heuristic one); index < 0 restores the autotuner. */
int  yn_set_pw_config(yn_handle* h, int index);
/* The process-wide autotune table (layer shape -> tile configuration) of `device` to / from a small text file, the device ordinal
 * left out: the ranks of a multi-GPU job adopt ONE rank's choices instead of each timing the same shapes at once (bench.py).
 * yn_tune_load returns the number of entries adopted (existing ones are kept), -1 if the file cannot be read. */
int  yn_tune_save(const char* path, int device);
int  yn_tune_load(const char* path, int device);
int  yn_pw_config_count(void);
/* Configurations [0, yn_pw_f32_config_count()) are the f32-MFMA family (LDS-tiled, then register-direct), the rest the split-f16
 * family (gemm_split_kernel); results are bit-identical INSIDE a family. */
int  yn_pw_f32_config_count(void);
/* The stride-1 ShuffleV2 units run as one kernel each (depthwise -> pw2 -> concat+shuffle -> next unit's pw1).  mode 1
 * (default): on the stages whose map is large enough for that to pay; 0: three kernels per unit everywhere; 2: one kernel per
 * unit everywhere.  All three give bit-identical results (A/B measurements, tests). */
int  yn_unit_chain(yn_handle* h, int mode);
/* The form of that one-kernel-per-unit launch (backbone/shufflenetv2.py:53-63, 70-72): unit_pipe_kernel, the persistent software-pipelined
 * tile walk - mode 1 (default): by its size rule; 0: never (unit_chain2_kernel everywhere); 2: also for few tiles.  Bit-identical. */
int  yn_chain_pipe(yn_handle* h, int mode);
/* All but the last stride-1 unit of a backbone stage (backbone/shufflenetv2.py:118-125: the `for i in range(numrepeat)` loop) as ONE
 * persistent launch (stage_pipe_kernel: (unit, tile) work items by ticket, tile-level ready flags between the units).  mode 1 (default):
 * from 256 tiles; 0: one launch per unit; 2: at every size.  publish_early 0 (default): a tile raises its ready flag under the next tile's
 * depthwise phase (at once when the workgroup has to wait for its next item's inputs); 1: right behind its stores.  Bit-identical to the
 * per-unit launches. */
int  yn_stage_fuse(yn_handle* h, int mode, int publish_early);
/* pw_pipe_kernel (the persistent form of a pointwise conv, utils/modules.py:8-18 folded) among the autotuner's candidates: 1 (default) / 0. */
int  yn_pw_pipe(yn_handle* h, int enable);

/* ---- weights ------------------------------------------------------------------------------- */
/* nn.Module.load_state_dict (eval.py:127, benchmark.py:132): one call per state-dict entry, using
 * the reference's 469 key names; `host_ptr` float32 (int64 for num_batches_tracked, ignored).   */
int  yn_load_param(yn_handle* h, const char* state_dict_key, const void* host_ptr,
                   const int64_t* shape, int ndim);
/* Same, source already in HBM (e.g. a torch Parameter's data_ptr()). */
int  yn_load_param_dev(yn_handle* h, const char* state_dict_key, const void* dev_ptr,
                       const int64_t* shape, int ndim);
/* utils/fuse_conv_bn.py:6-53 — fold every BN into its conv and repack for the kernels.  Must be
 * called after loading parameters and before inference.  A conv whose BN keys were never loaded
 * is taken as already folded (the state dict of a model that went through fuse_conv_bn()).      */
int  yn_fold_bn(yn_handle* h);
/* Read back the folded weight/bias of one conv in the reference layout [Cout,Cin/g,k,k] / [Cout]
 * (parity check of utils/fuse_conv_bn.py:17-21). `conv_key` e.g. "smooth_1.convs.0".           */
int  yn_get_folded(yn_handle* h, const char* conv_key, float* host_weight, float* host_bias);

/* ---- the network --------------------------------------------------------------------------- */
/* YOLONano.forward lines 284-301: backbone, FPN+PAN neck, three heads.  x_dev: NCHW
 * [B,3,S,S] float32.  Outputs: NHWC raw head tensors [B,S/8,S/8,A(5+C)], [B,S/16,..], [B,S/32,..]. */
int  yn_forward_raw(yn_handle* h, const float* x_dev, int B,
                    float* head_s8_dev, float* head_s16_dev, float* head_s32_dev);

/* ShuffleNetV2.forward (backbone/shufflenetv2.py:157-167): the same network pass, additionally copying the three backbone
 * taps the neck consumes — c3 [B,S/8,S/8,C3], c4 [B,S/16,S/16,C4], c5 [B,S/32,S/32,C5], NHWC float32 (C = 116/232/464 for
 * 1.0x, 48/96/192 for 0.5x) — so that a backbone failure localises (parity tests; never graph-captured). */
int  yn_forward_taps(yn_handle* h, const float* x_dev, int B, float* c3_dev, float* c4_dev, float* c5_dev);

/* Lines 308-330 + 362-367 for EVERY image of the batch (the reference only finishes image 0):
 * all_bbox [B,N,4] = clamp(decode_boxes/S, 0, 1); all_class [B,N,C] = softmax(cls)*sigmoid(obj). */
int  yn_score_full(yn_handle* h, const float* head_s8_dev, const float* head_s16_dev,
                   const float* head_s32_dev, int B, float* all_bbox_dev, float* all_class_dev);

/* YOLONano.decode_boxes :139-156 — txtytwth [B, sum HW, A, 4] -> xyxy pixels [B, N, 4]. */
int  yn_decode_boxes(yn_handle* h, const float* txtytwth_dev, int B, float* xyxy_dev);

/* YOLONano.create_grid :86-112 — host arrays grid [HWtot,2], stride [HWtot,A,2], anchors [HWtot,A,2]. */
int  yn_create_grid(yn_handle* h, int input_size, float* grid_host, float* stride_host, float* anchor_host);
/* the same for a height x width canvas: cells of a scale in row order, gy * (width/st) + gx */
int  yn_create_grid_rect(yn_handle* h, int height, int width, float* grid_host, float* stride_host, float* anchor_host);

/* ---- post-processing ----------------------------------------------------------------------- */
/* YOLONano.nms :159-188 / diou_nms :191-242 — one class.  dets [n,4] xyxy, scores [n]; writes the
 * kept indices in pick order (descending score; equal scores: higher index first) and the count. */
int  yn_nms(yn_handle* h, const float* dets_dev, const float* scores_dev, int n, float nms_thresh,
            int diou, int32_t* keep_dev, int32_t* count_dev);

/* Per-class NMS over an arbitrary detection list — the merge step of TestTimeAugmentation (utils/misc.py:132-146, nms of
 * utils/misc.py:8-37 = the arithmetic of YOLONano.nms): boxes [n,4], scores [n], cls [n] (0 <= cls < num_classes) ->
 * kept detections in ascending input order, count[0] = K.  Output buffers have capacity n. */
int  yn_nms_merge(yn_handle* h, const float* boxes_dev, const float* scores_dev, const int32_t* cls_dev, int n, int num_classes,
                  float nms_thresh, int diou, float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index, int32_t* count_dev);

/* Weighted box fusion over an arbitrary detection list - the twin of yn_nms_merge, and the second merge rule of yn_tta / yn_slice / yn_fuse
 * (DESIGN.md 30 is the specification; tests/wbf_oracle.py restates it in float32 numpy and the kernel agrees bit for bit).  The rule is
 * this package's own: parity with the ensemble_boxes family is UNPINNED.  Per class, rows are visited in yn_nms_merge's pick order (score
 * descending, higher row first among equals).  A row joins the cluster whose FUSED box has the largest ovr with it among those with
 * ovr > iou_thresh (strict; NaN never matches; equal ovr: the earliest cluster) - ovr in yn_nms_merge's arithmetic - and then
 * n += 1, S += s, P[j] += s * b[j], fused[j] = P[j] / S; otherwise it founds a cluster whose fused box is its own box bit for bit.
 * Every operation is one float32 operation.  Delivered per cluster, in ascending order of the founder's row: fused box, score
 * (S / (float)n) * ((float)min(n, expected) / (float)expected), class, founder row (out_index), votes n (out_votes).  assign_dev [n] (may
 * be NULL): per input row the founder row of the cluster it ended in (-1 for a row of class -1).  out_index / out_votes may be NULL.
 * Output buffers have capacity n; count_dev[0] = clusters.  Refused, each by name: expected < 1, n < 0, num_classes other than the
 * handle's.  n == 0 is an empty result.  No segment length is refused: clusters past yn_wbf_lds_clusters() live in device memory. */
int  yn_wbf_merge(yn_handle* h, const float* boxes_dev, const float* scores_dev, const int32_t* cls_dev, int n, int num_classes,
                  float iou_thresh, int expected, float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index,
                  int32_t* out_votes, int32_t* assign_dev, int32_t* count_dev);
/* clusters of one (list, class) segment whose state the kernel keeps in LDS (a testing aid: cases straddle it) */
int  yn_wbf_lds_clusters(void);
/* the documented cost model: the most 64-lane steps the walk of a segment of n_rows rows ending in n_clusters clusters takes */
int64_t yn_wbf_cost(int64_t n_rows, int64_t n_clusters);
/* the merge rules of yn_tta / yn_slice / yn_fuse */
enum { YN_MERGE_NMS = 0, YN_MERGE_WBF = 1 };

/* ---- Soft-NMS (after Bodla et al., 2017): the per-class NMS with another suppression function.  A neighbour of a kept box is not dropped
 * but has its score marked down by a function of the overlap (DESIGN.md 31 is the specification; tests/soft_nms_oracle.py restates it in
 * float32 numpy and the kernel agrees bit for bit).  The rule is this package's own: parity with any third-party Soft-NMS is UNPINNED.
 * It is NOT a third merge rule: it is how the YN_MERGE_NMS rule (and the NMS inside yn_infer / yn_postprocess) suppresses.
 * Per (list, class) segment: the live rows are those with score > score_floor (strict: a NaN score is never live).  While a row is live,
 * the live row with the largest CURRENT score is picked (equal scores: the higher row), kept with that score and taken out; every other
 * live row's score is multiplied (one float32 multiply) by w(ovr), ovr in yn_nms_merge's arithmetic against the picked box (never DIoU),
 * hit = !(ovr <= iou_thresh) (a NaN hits):
 *     YN_SOFT_HARD      w = hit ? 0 : 1
 *     YN_SOFT_LINEAR    w = hit ? 1 - ovr : 1
 *     YN_SOFT_GAUSSIAN  w = E(-((ovr * ovr) / sigma)) for every row (iou_thresh is not used); E is the package's own float32 exp
 * and the row leaves the live set unless its new score is > score_floor.  Kept rows are delivered in ascending row order: the box bit for
 * bit, the decayed score, the class, the row.  With YN_SOFT_HARD, score_floor 0 and positive scores the result is yn_nms_merge's. */
enum { YN_SOFT_OFF = 0, YN_SOFT_HARD = 1, YN_SOFT_LINEAR = 2, YN_SOFT_GAUSSIAN = 3 };
/* The twin of yn_nms_merge / yn_wbf_merge, with their conventions: output buffers have capacity n, out_index may be NULL, n == 0 is an
 * empty result, count_dev[0] = kept rows.  Refused, each by name: a method outside 1..3, a sigma that is not positive and finite, a
 * score_floor that is negative or not finite, n < 0, num_classes other than the handle's.  No segment length is refused: the scores of
 * rows past yn_soft_lds_rows() live in device memory. */
int  yn_soft_nms_merge(yn_handle* h, const float* boxes_dev, const float* scores_dev, const int32_t* cls_dev, int n, int num_classes,
                       int method, float iou_thresh, float sigma, float score_floor, float* out_boxes, float* out_scores, int32_t* out_cls,
                       int32_t* out_index, int32_t* count_dev);
/* How the per-class NMS inside yn_infer and yn_postprocess suppresses from now on.  YN_SOFT_OFF (the default) is the NMS chain, launch for
 * launch; any other method runs the Soft-NMS route at the handle's nms_thresh with the same output layout and capacity (scores are the
 * decayed ones).  Use the handle's conf_thresh as score_floor to keep the delivered scores at or above it.  A change drops the captured
 * graphs.  With diou_nms set on the handle and a method other than OFF, yn_infer / yn_postprocess refuse by name: Soft-NMS has no DIoU
 * form here.  yn_nms, yn_nms_merge and yn_nms_stages are not affected. */
int  yn_soft_nms(yn_handle* h, int method, float sigma, float score_floor);
/* rows of one (list, class) segment whose state the kernel keeps in LDS (a testing aid: cases straddle it) */
int  yn_soft_lds_rows(void);
/* testing aid: y_dev[i] = E(x_dev[i]) for n floats - the exp of YN_SOFT_GAUSSIAN on its own (E(NaN) = NaN, E(x < -87) = 0) */
int  yn_op_soft_exp(yn_handle* h, const float* x_dev, float* y_dev, int64_t n);

/* ValTransforms (data/transforms.py:445-458 = Resize :73-119 + Normalize :59-70 + ToTensor :394-398; call sites
 * benchmark.py:58, evaluator/vocapi_evaluator.py:64): img_dev = uint8 [h0][w0][3] BGR on the device -> x_dev float32
 * [3][side][side] RGB, normalised, letterboxed.  The caller supplies Resize's integer geometry (rw x rh resized extent placed
 * at (left, top) inside the side x side square, padded with mean*255) — it is host arithmetic the reference does in Python
 * (`int(r * size)`, `//`); the resize itself is cv2's 8-bit INTER_LINEAR.  mean / std: 3 host floats each, BGR order. */
int  yn_preprocess(yn_handle* h, const uint8_t* img_dev, int h0, int w0, int rw, int rh, int left, int top, int side,
                   const float* mean_host, const float* std_host, float* x_dev);

/* The same for n images in one launch per 32: imgs_host[i] = device pointer of image i, geom_host[i] = {h0, w0, rw, rh, left,
 * top}; x_dev = float32 [n][3][side][side] (the network's input batch). */
int  yn_preprocess_batch(yn_handle* h, int n, const uint8_t* const* imgs_host, const int32_t* geom_host, int side,
                         const float* mean_host, const float* std_host, float* x_dev);

/* The win_w x win_h window at (win_left, win_top) of the tensor yn_preprocess_batch would write for the same arguments (the input of a
 * yn_set_grid_rect grid): x_dev = float32 [n][3][win_h][win_w], the same resize arithmetic, pad value and normalise order, bit for bit.
 * A window that cuts into any image's resized extent [left_i, left_i + rw_i) x [top_i, top_i + rh_i) is refused: only pad may be cut off. */
int  yn_preprocess_batch_rect(yn_handle* h, int n, const uint8_t* const* imgs_host, const int32_t* geom_host, int side,
                              int win_left, int win_top, int win_w, int win_h,
                              const float* mean_host, const float* std_host, float* x_dev);

/* TrainTransforms / ColorTransforms pixel work (data/transforms.py:402-442; call site data/voc.py:231), n images in one launch per
 * 32: imgs_host[i] = device pointer of frame i, uint8 [h0][w0][3] BGR as cv2.imread gives it -> x_dev float32 [n][3][side][side]
 * RGB (the network's input batch).  Every random draw and all box arithmetic stay on the host (yolo_nano_amd.TrainTransforms.sample
 * restates them); per image the device gets
 *   geom_host[12*i + ...]  int32  0 h0, 1 w0       frame shape (ToAbsoluteCoords :122-130)
 *                                 2 x, 3 y, 4 w, 5 h   crop (RandomSampleCrop :285-287: rect[0], rect[1], rect[2] - rect[0],
 *                                                  rect[3] - rect[1]); the uncropped image is 0, 0, w0, h0
 *                                 6 mirror          RandomMirror :312 fired (image[:, ::-1] of the crop)
 *                                 7 rw, 8 rh        Resize :79-111 resized extent of the w x h crop (`int(r * size)`)
 *                                 9 left, 10 top    its place inside the side x side square (`dw // 2`, `dh // 2`)
 *                                 11 flags          YN_AUG_* bits: which photometric draws fired, and the branch (:365-368)
 *   photo_host[7*i + ...]  float  0 brightness delta (:222), 1 contrast alpha (:209), 2 saturation factor (:147), 3 hue delta
 *                                 (:160), each float32(u) of the float64 draw (unused unless its flag is set);
 *                                 4..6 letterbox pad, BGR: float32(float64(mean[c]) * 255) (Resize.mean :76)
 * The chain runs per pixel in the reference's order: brightness, then [contrast,] BGR->HSV, saturation, hue, HSV->BGR [, contrast],
 * nothing clipped; the resize is cv2's float INTER_LINEAR (area fast path for an exact 2:1 reduction, copy when w x h = rw x rh);
 * Normalize uses mean_host / std_host: 3 host floats each, BGR order.  n == 0 is not an error. */
#define YN_AUG_BRIGHTNESS     1   /* RandomBrightness fired */
#define YN_AUG_CONTRAST       2   /* RandomContrast fired */
#define YN_AUG_CONTRAST_FIRST 4   /* PhotometricDistort drew pd[:-1] (contrast before HSV); clear: pd[1:] (contrast after BGR) */
#define YN_AUG_SATURATION     8   /* RandomSaturation fired */
#define YN_AUG_HUE            16  /* RandomHue fired */
int  yn_train_transform_batch(yn_handle* h, int n, const uint8_t* const* imgs_host, const int32_t* geom_host, const float* photo_host,
                              int side, const float* mean_host, const float* std_host, float* x_dev);

/* Mosaic samples (data/voc.py:140-211 load_mosaic, then ColorTransforms data/transforms.py:424-442; call site data/voc.py:216-220),
 * n mosaics in one launch per 14 (the descriptors travel in the kernel arguments): imgs_host[4*i + k] = device pointer of frame k of
 * mosaic i, uint8 [h0][w0][3] BGR -> x_dev float32 [n][3][side][side] RGB.  The 2*mosaic_size square canvas is never built: every
 * canvas pixel is computed where the Resize of the canvas reads it.  Every draw and all box arithmetic stay on the host
 * (yolo_nano_amd.Mosaic.sample restates them); per mosaic the device gets
 *   geom_host[50*i + 12*k + ...]  int32, frame k = 0..3 in load_mosaic's order (top left, top right, bottom left, bottom right)
 *                                 0 h0, 1 w0        frame shape (:165)
 *                                 2 rw, 3 rh        cv2.resize extent `(int(w0 * r), int(h0 * r))`, r = mosaic_size / max(h0, w0)
 *                                                   (:168-171); w0, h0 when r == 1 (the frame is then pasted unresized)
 *                                 4 x1a, 5 y1a, 6 x2a, 7 y2a     canvas rectangle `mosaic_img[y1a:y2a, x1a:x2a]` (:175-187)
 *                                 8 x1b, 9 y1b, 10 x2b, 11 y2b   source rectangle `img_i[y1b:y2b, x1b:x2b]` of the resized frame, same size
 *   geom_host[50*i + 48]          mirror: RandomMirror :312 fired on the canvas (`image[:, ::-1]`)
 *   geom_host[50*i + 49]          flags: YN_AUG_* bits, as for yn_train_transform_batch
 *   photo_host[7*i + ...]  float  0..3 the four photometric factors as for yn_train_transform_batch; 4..6 canvas fill, BGR:
 *                                 float32(float64(mean[c]) * 255) (:155-156: the canvas is float64, ConvertFromInts makes it float32)
 * The frame resize is cv2's 8-bit INTER_LINEAR (as yn_preprocess: copy when the extent is the frame's, the area fast path for an
 * exact 2:1 reduction); the photometric chain then runs on every canvas pixel, the fill included (unlike Resize's letterbox pad,
 * the fill is part of the image PhotometricDistort sees); the canvas goes to side x side with cv2's float INTER_LINEAR (area fast
 * path when 2*mosaic_size == 2*side, copy when 2*mosaic_size == side).  A frame pasted later overwrites an earlier one.
 * Refused before anything is launched, with yn_last_error naming the mosaic and frame: null pointers, non-positive extents, a
 * canvas rectangle outside [0, 2*mosaic_size], a source rectangle outside the resized frame, rectangle sizes that differ, bad
 * mirror / flags, non-positive std.  n == 0 is not an error. */
int  yn_mosaic_transform_batch(yn_handle* h, int n, const uint8_t* const* imgs_host, const int32_t* geom_host, const float* photo_host,
                               int mosaic_size, int side, const float* mean_host, const float* std_host, float* x_dev);

/* YOLONano.postprocess :245-279, batched: all_local [B,N,4], all_conf [B,N,C] ->
 * per image b: count[b] = K_b and, in ascending candidate order, out_boxes[b,0:K_b,4],
 * out_scores[b,0:K_b], out_cls[b,0:K_b], out_index[b,0:K_b] (candidate index; may be NULL).
 * Output buffers have capacity N per image. */
int  yn_postprocess(yn_handle* h, const float* all_local_dev, const float* all_conf_dev, int B, int N, int C,
                    float* out_boxes_dev, float* out_scores_dev, int32_t* out_cls_dev,
                    int32_t* out_index_dev, int32_t* count_dev);

/* The whole eval-mode YOLONano.forward :282-376 for a batch: network + score head + per-class NMS,
 * all on device, no host round trip.  Outputs as yn_postprocess. */
int  yn_infer(yn_handle* h, const float* x_dev, int B,
              float* out_boxes_dev, float* out_scores_dev, int32_t* out_cls_dev,
              int32_t* out_index_dev, int32_t* count_dev);

/* The hand-over that ends YOLONano.forward (`.to('cpu').numpy()`, models/yolo_nano.py:370-376) for a whole batch: gathers the
 * kept rows of the yn_infer / yn_postprocess outputs of all B images into ONE contiguous record list
 * rec_dev [total][6] float32 = x1, y1, x2, y2, score, class (image order; ascending candidate order inside an image; the class
 * as a float, exact below 2^24) and offsets_dev[B+1] = exclusive prefix of the counts ([B] = total).  The host then needs two
 * copies per batch (the offsets, then total*24 bytes) instead of three per image.  rec_dev has capacity B*N records. */
int  yn_pack_detections(yn_handle* h, const float* out_boxes_dev, const float* out_scores_dev, const int32_t* out_cls_dev,
                        const int32_t* count_dev, int B, int N, float* rec_dev, int32_t* offsets_dev);

/* ---- VOC mAP: VOCAPIEvaluator.evaluate + do_python_eval (evaluator/vocapi_evaluator.py:56-198, voc_eval :233-338, voc_ap :199-230)
 * on the device, bit for bit with the reference's numpy arithmetic (DESIGN.md §VOC mAP).  The evaluator is an object of its own, so it
 * outlives any handle; every call launches on the stream of the handle it is given.  Per class, detections are ordered by score
 * descending and, among equal 3-decimal scores, in file order (image in add order, then position in the image's record list): the
 * reference's np.argsort is unstable there, the one point where it is not deterministic. */
typedef struct yn_eval yn_eval;
/* num_classes 1..2000, ovthresh = voc_eval's ovthresh (a strict >) */
int  yn_eval_create(yn_handle* h, int num_classes, double ovthresh, yn_eval** out);
void yn_eval_destroy(yn_eval* e);
/* drops every image, record and ground-truth box added so far */
int  yn_eval_reset(yn_handle* h, yn_eval* e);
/* B images: rec_dev / offsets_dev as yn_pack_detections wrote them (device; normalised boxes of the letterboxed square), geom_host
 * int32 [B][7] = w0, h0, rw, rh, left, top, side (the letterbox geometry, ValTransforms.geometry), gt_host int32 [G][6] = x1, y1, x2,
 * y2, class, difficult (the VOC XML integers, parse_rec :100-117) with gt_offsets_host [B+1].  Reads offsets_dev[B] to size the
 * store (one 4-byte read-back, synchronises the stream); a negative total (the split-f16 range mark) returns YN_STATUS_RANGE and
 * adds nothing.  Records are mapped to image pixels and through the reference's text-file route (score to 3 decimals, box + 1 to
 * 1 decimal) on the device.  At most 4096 ground-truth boxes per (image, class), 2^22 records per image, 2^21 images. */
int  yn_eval_add(yn_handle* h, yn_eval* e, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom_host,
                 const int32_t* gt_host, const int32_t* gt_offsets_host);
/* per-class AP into ap_host [C] (-1 for a class without detections, as :334-336; use_07_metric: 11-point, else area), non-difficult
 * ground truth npos_host [C] and detections ndet_host [C] (either may be NULL).  mAP = np.mean(ap) is the caller's.  Fails, naming
 * it, if an added record had a score outside 0.000..1.000 after rounding, a class outside 0..C-1 or a non-finite coordinate. */
int  yn_eval_finish(yn_handle* h, yn_eval* e, int use_07_metric, double* ap_host, int64_t* npos_host, int64_t* ndet_host);
/* after yn_eval_finish: the first min(ndet, cap) points of class cls's rec / prec arrays (:328-333); either pointer may be NULL */
int  yn_eval_curve(yn_handle* h, yn_eval* e, int cls, double* rec_host, double* prec_host, int64_t cap);
/* testing aid: the first min(n, cap) ingested records as host int32 [n][7] = image, class, score bin k (score = k / 1000), x1, y1,
 * x2, y2 in tenths (coordinate + 1 = tenths / 10), in ingest order */
int  yn_eval_records(yn_handle* h, yn_eval* e, int32_t* host, int64_t cap);
/* records and images added so far (host counters, no device work) */
int  yn_eval_size(yn_eval* e, int64_t* records, int64_t* images);

/* ---- COCO box AP: what evaluator/cocoapi_evaluator.py:85-130 obtains from pycocotools' COCOeval(iouType 'bbox') - computeIoU,
 * evaluateImg and accumulate on the device (COCO box AP); summarize, 12 means over the two arrays, is the caller's
 * (yolo_nano_amd.coco does it in numpy).  An object of its own like yn_eval; every call launches on the stream of the handle given.
 * All orders are COCOeval's stable ones: by score descending; inside an image equal scores in results-list order; between images
 * equal scores in ascending image id.  Parity with pycocotools itself is unpinned where the library cannot be installed; the
 * host restatement tests/coco_oracle.py is what the device is tested against, bit for bit. */
typedef struct yn_coco yn_coco;
/* num_classes 1..2000 (all are evaluated), max_det = the last entry of maxDets (100), 1..1023: what is kept per (image, category) */
int  yn_coco_create(yn_handle* h, int num_classes, int max_det, yn_coco** out);
void yn_coco_destroy(yn_coco* e);
/* drops every image, detection and ground-truth box added so far */
int  yn_coco_reset(yn_handle* h, yn_coco* e);
/* B images: rec_dev / offsets_dev as yn_pack_detections wrote them (device), geom_host int32 [B][7] as for yn_eval_add,
 * image_ids_host int64 [B], gt_host float64 [G][5] = x, y, w, h, area (area as the annotation file gives it), gt_meta_host int32
 * [G][2] = category index, iscrowd, gt_offsets_host [B+1].  Boxes are mapped to image pixels in the evaluator's float32 steps;
 * per (image, category) the max_det best by score are kept (float32 x1, y1, x2, y2, score), so the store is bounded by
 * max_det * num_classes per image.  Two 4-byte read-backs; a negative offsets[B] (the split-f16 range mark) returns
 * YN_STATUS_RANGE and adds nothing.  Limits, each refused by name: 4096 ground-truth boxes per (image, category), 2^21 images,
 * 2^31 - 1 detections kept and ground-truth boxes in all; non-finite ground truth or a category outside 0..C-1 fails here. */
int  yn_coco_add(yn_handle* h, yn_coco* e, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom_host,
                 const int64_t* image_ids_host, const double* gt_host, const int32_t* gt_meta_host, const int32_t* gt_offsets_host);
/* The parameters are the caller's doubles (numpy's linspace values), never recomputed: iou_thrs [num_iou <= 10], rec_thrs
 * [num_rec <= 256, ascending], area_rng [num_area <= 4][2], max_dets [num_max_dets <= 8, ascending, last == max_det].
 * precision_host [num_iou][num_rec][C][num_area][num_max_dets] and recall_host [num_iou][C][num_area][num_max_dets] in
 * COCOeval's layout, -1 where a category has no non-ignored ground truth.  Fails, naming it, if an image id was added twice or a
 * detection had a non-finite coordinate or score or a category outside 0..C-1. */
int  yn_coco_finish(yn_handle* h, yn_coco* e, const double* iou_thrs_host, int num_iou, const double* rec_thrs_host, int num_rec,
                    const double* area_rng_host, int num_area, const int32_t* max_dets_host, int num_max_dets, double* precision_host,
                    double* recall_host);
/* testing aid, after yn_coco_finish: the store det_host [n][5] = x1, y1, x2, y2, score; seg_host [images * C + 1] = where the
 * detections of (image in add order, category) start, in rank order; flags_host [num_area][n] with bit t = matched at IoU
 * threshold t and bit 16 + t = ignored at it.  Any pointer may be NULL. */
int  yn_coco_matches(yn_handle* h, yn_coco* e, float* det_host, int64_t* seg_host, uint32_t* flags_host, int num_area);
/* detections kept and images added so far (host counters, no device work) */
int  yn_coco_size(yn_coco* e, int64_t* detections, int64_t* images);

/* ---- anchor-box k-means: kmeans_anchor.py's init_centroids / do_kmeans / anchor_box_kmeans on the device, in float64 with exact sums
 * (Anchor k-means).  Boxes are (w, h) pairs centred at the origin; the distance is 1 - IoU in the reference's operation
 * order; every sum (group sums, loss, the k-means++ prefix sums) is the correctly rounded exact sum, so a result does not depend on
 * box order, grid or timing.  Domain: 1 <= w, h < 65536, finite.  An object of its own like yn_coco; every call launches on the
 * stream of the handle given.  N is bounded by the limb layout of the pass: 256 workgroups of at most 2^16 boxes each, whose 47-bit
 * limbs fit a 64-bit accumulator, which is 2^24 boxes. */
typedef struct yn_kmeans yn_kmeans;
/* capacity 1..2^24 boxes, max_k 1..32 centroids */
int  yn_kmeans_create(yn_handle* h, int64_t capacity, int max_k, yn_kmeans** out);
void yn_kmeans_destroy(yn_kmeans* e);
/* wh_dev float64 [n][2] on the device, copied into the object; fails, giving their number, if any box lies outside the domain
 * (one read-back).  Drops the centroids. */
int  yn_kmeans_set_boxes(yn_handle* h, yn_kmeans* e, const double* wh_dev, int64_t n);
/* k-means++ as init_centroids: centroid 0 is box first_index; for centroid r = 1..k-1 the pick is the first index whose exact prefix
 * sum of min_distance exceeds sum_distance * u_host[r-1] (the caller's uniform draws in [0, 1), in the reference's order), or no box
 * (picked -1, centroid (0, 0)) if no index qualifies.  centroids_host float64 [k][2], picked_host int32 [k]; either may be NULL.
 * One read-back per round. */
int  yn_kmeans_seed(yn_handle* h, yn_kmeans* e, int k, int64_t first_index, const double* u_host, double* centroids_host,
                    int32_t* picked_host);
/* wh_host float64 [k][2], each side finite and in [0, 65536) */
int  yn_kmeans_set_centroids(yn_handle* h, yn_kmeans* e, const double* wh_host, int k);
/* anchor_box_kmeans's loop from the current centroids: passes until |old_loss - loss| < loss_convergence or iterations > iters,
 * decided on the device; the host enqueues passes in batches and reads the `done` word once per batch.  centroids_host [k][2],
 * counts_host int64 [k], loss_host, iterations_host of the last pass; any may be NULL. */
int  yn_kmeans_run(yn_handle* h, yn_kmeans* e, double loss_convergence, int iters, double* centroids_host, int64_t* counts_host,
                   double* loss_host, int32_t* iterations_host);
/* one do_kmeans: the current centroids are replaced by their groups' means; outputs as yn_kmeans_run's */
int  yn_kmeans_pass(yn_handle* h, yn_kmeans* e, double* centroids_host, int64_t* counts_host, double* loss_host);
/* group_dev int32 [n] on the device: the group of every box for the current centroids (ties to the lower index).  Asynchronous. */
int  yn_kmeans_assign(yn_handle* h, yn_kmeans* e, int32_t* group_dev);
/* passes run and host reads made by the last yn_kmeans_run (host counters, no device work) */
int  yn_kmeans_stats(yn_kmeans* e, int64_t* passes, int64_t* host_reads);

/* ---- test-time augmentation for whole batches: utils/misc.py:90-148 (TestTimeAugmentation) for B images at once, nothing but one
 * small read-back crossing to the host (Test-time augmentation).  An object of its own like yn_coco; every call launches on
 * the stream of the handle given.
 *
 * The bilinear resize (F.interpolate, mode 'bilinear', align_corners False, no antialias; :108-111) is DEFINED here, since torch's own
 * kernel is not reproducible bit for bit across thread counts.  Per axis, scale = (float)S0 / (float)s;
 * src = max(fmaf(scale, d + 0.5f, -0.5f), 0) with one rounding; i0 = (int)src, i1 = i0 + (i0 < S0 - 1); l1 = src - i0, l0 = 1 - l1;
 * v = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d), every multiply and add rounded on its own.  s == S0 copies the bits.
 * tests/tta_oracle.py restates it in numpy; the distance to torch is bounded in tests/test_tta_cpu.py. */
/* x_dev float32 [B][3][S0][S0] -> out_dev [B][3][s][s], or with flip_pairs [2B][3][s][s]: image 2b the resize of image b, image
 * 2b + 1 its horizontal mirror (out[..., j] = resized[..., s - 1 - j], torch.flip(x, [-1])).  Any sides 1..16384 (the network's
 * multiple-of-32 rule is yn_set_grid's, not this call's); B == 0 does nothing.  Asynchronous.  Also the F.interpolate of multi-scale
 * training (train.py:202-208). */
int  yn_resize_batch(yn_handle* h, const float* x_dev, int B, int S0, int s, int flip_pairs, float* out_dev);
typedef struct yn_tta yn_tta;
/* scales: ascending positive multiples of 32 (num_scales 1..64; np.arange(320, 641, 32) is the reference's default); flip: also the
 * mirrored forward of every scale; max_batch: images per call; list_capacity: rows of an image's merge list, 1..131072 - the sum
 * over all forwards of what yn_infer keeps for that image.  Every work buffer is allocated here, for max_batch images and the
 * largest scale.  The handle gives the device, the anchors per cell and the class count. */
int  yn_tta_create(yn_handle* h, const int32_t* scales, int num_scales, int flip, int max_batch, int list_capacity, yn_tta** out);
void yn_tta_destroy(yn_tta* t);
/* x_dev float32 [B][3][S0][S0].  Per scale s, ascending: one resize (+ mirror) launch, yn_set_grid(s), ONE yn_infer over the 2B (B
 * without flip) images on the handle's own path and thresholds, one append of every image's kept rows to its merge list - plain rows
 * copied, mirrored rows with x1' = 1.0f - x2, x2' = 1.0f - x1 (:126).  List order is the reference's concatenation order: scale by
 * scale, plain before mirrored, ascending candidate order inside a forward.  Then the merge of the B lists, the one yn_slice_merge
 * documents below (nms_thresh; the reference uses 0.4): yn_tta and yn_slice hold the same merge lists, state words and result
 * (DESIGN.md 28 describes them once).  The grid that was set before the call is restored, also on failure.
 * Needs a handle created with max_batch >= 2B (B without flip), refused by name otherwise.  A forward that left the split-f16 range
 * returns YN_STATUS_RANGE and delivers nothing (acknowledge with yn_range_status, yn_exact_f32(h, 1), run again).  A list that would
 * pass list_capacity fails, naming the first such image and the rows it needed; nothing is written past a list.  B == 0 is an empty
 * result, not an error. */
int  yn_tta_infer(yn_handle* h, yn_tta* t, const float* x_dev, int B, int S0, float nms_thresh);
/* The rule yn_tta_infer's merge applies from now on: YN_MERGE_NMS (the default) or YN_MERGE_WBF (yn_wbf_merge's rule per list; the float
 * argument of yn_tta_infer is then its iou_thresh).  expected: the expected votes, 0 = the object's default, its number of forwards. */
int  yn_merge_rule_tta(yn_handle* h, yn_tta* t, int rule, int expected);
/* the last successful yn_tta_infer's result, owned by the object and valid until its next call: rec_dev [total][6] + offsets_dev
 * [B+1], exactly yn_pack_detections' layout (what yn_eval_add / yn_coco_add take).  Any pointer may be NULL; asking for `total` costs
 * one 4-byte read-back (once per result).  Returns 1 when there is no result. */
int  yn_tta_result(yn_tta* t, const float** rec_dev, const int32_t** offsets_dev, int32_t* total);
/* testing aid: the merge lists of the last yn_tta_infer (also one that failed on list_capacity) before the NMS, to the host:
 * boxes_host [B][list_capacity][4], scores_host / cls_host [B][list_capacity] (rows >= count: class -1), count_host [B] (the rows the
 * list needed, which may exceed list_capacity) and forward_start_host [forwards][B], forwards = (flip ? 2 : 1) * num_scales in list
 * order: where forward f's rows start in image b's list.  Any pointer may be NULL.  Synchronises the stream. */
int  yn_tta_forwards(yn_handle* h, yn_tta* t, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host,
                     int32_t* forward_start_host);

/* ---- sliced inference: a frame larger than the network input runs as overlapping tiles at native resolution, plus the whole frame once;
 * every tile's boxes go back into the frame and are merged per frame with per-class NMS (DESIGN.md 28 is the specification;
 * yolo_nano_amd.slicing.slice_grid / tile_table build the table).  Frames are uint8 [h0][w0][3] BGR on the device, rows contiguous, sides
 * 1..16384: frames_host[f] = device pointer of frame f, shapes_host[f] = {h0, w0}.  The tile table tiles_host [T][9] is int32 rows
 * frame, x, y, tw, th, rw, rh, left, top: the rectangle frame[y:y+th, x:x+tw], and Resize's integer geometry of that rectangle taken as an
 * image (what yn_preprocess_batch takes as rw, rh, left, top).  Every entry checks the rows it reads before anything is launched and
 * refuses, naming the tile: a frame index outside the frames, a rectangle outside its frame, non-positive extents, a letterbox geometry
 * outside the side x side square.  The object stands on its own, as yn_tta does, and launches on the stream of the handle passed. */
typedef struct yn_slice yn_slice;
/* max_frames: frames per call (1..4096); list_capacity: rows of one frame's merge list, 1..131072 - the sum over the frame's tiles of what
 * yn_infer keeps (after the edge filter).  The lists and the result are allocated here; the tile batch of yn_slice_infer follows the
 * handle's grid and max_batch at its first call.  The handle gives the device, the anchors per cell and the class count. */
int  yn_slice_create(yn_handle* h, int max_frames, int list_capacity, yn_slice** out);
void yn_slice_destroy(yn_slice* s);
/* The tile kernel on its own: x_dev float32 [T][3][side][side]; tile t holds, bit for bit, what yn_preprocess_batch writes for a
 * contiguous copy of frame[y:y+th, x:x+tw] with geometry {th, tw, rw, rh, left, top} - the same cv2 8-bit INTER_LINEAR (a copy when the
 * extent is the tile's, the area path for an exact 2:1), the same pad and normalise order.  The frame is read in place by its row pitch
 * 3 * w0; no crop is made.  One launch per 64 tiles.  mean / std: 3 host floats each, BGR order.  Also refused: null pointers (a frame's
 * included), non-positive std.  The table's frame indices must lie inside frames_host / shapes_host (this entry has no frame count to
 * check them against; only negative ones are refused).  T == 0 does nothing.  Asynchronous.
 * On a tile with tw == th == rw == rh == side (side % 4 == 0, x_dev 16-byte aligned) the kernel loads the source as whole 4-byte-aligned
 * words: it may READ up to 3 bytes in front of the frame's first byte and up to 3 behind its last.  Such a word always holds a byte of
 * the frame, so it lies in the frame's page and the read cannot fault; nothing outside the frame is used or written.  A tool that
 * checks object bounds byte by byte would report it. */
int  yn_slice_preprocess(yn_handle* h, int T, const uint8_t* const* frames_host, const int32_t* shapes_host, const int32_t* tiles_host, int side,
                         const float* mean_host, const float* std_host, float* x_dev);
/* The kept rows of ONE yn_infer over tiles t0 .. t0 + n - 1 of the table (out_* and count_dev in yn_infer's layout, image j = tile t0 + j,
 * N = capacity per image) go to the end of their frames' merge lists.  A frame's list is in table order of its tiles, ascending candidate
 * order inside a tile, whatever the chunking: chunks must arrive in table order, t0 == 0 opens a new table (empties the F lists), any other
 * t0 must continue where the last chunk ended.  `side` of the geometry is the handle's current grid, which must be square.
 * A box b in [0,1] of the tile's square becomes
 *   p = bboxes -= offset; /= scale; *= size of the evaluators with the geometry {tw, th, rw, rh, left, top, side} (float64 operands, every
 *       step rounded to float32)
 *   q = p + (float)x for x1 / x2, p + (float)y for y1 / y2                                       one float32 add each
 *   edge filter, only when edge_margin m >= 0 (float32, every sum rounded once): the row is dropped if
 *       x > 0 && q.x1 < (float)x + m,  or  x + tw < w0 && q.x2 > (float)(x + tw) - m,  or the same two tests in y
 *     (a side that lies on the frame's edge never drops a box, so a full-frame tile is never filtered; strict compares: a box at
 *     exactly the margin stays)
 *   q clamped to [0, w0] (x) / [0, h0] (y):  q < 0 ? 0 : (q > hi ? hi : q)
 *   v = q / (float)max(h0, w0)                                                                     one float32 divide
 * Score and class are copied.  With the identity geometry row (w0, h0, w0, h0, 0, 0, max(h0, w0)) v is what yn_eval_add, yn_coco_add and
 * yn_draw_batch take.  A negative count (the split-f16 range mark) sets the object's range mark and appends none of that tile's rows.
 * Rows past list_capacity are counted, not written; the next yn_slice_merge fails on them.  out_boxes_dev must be 16-byte aligned (a
 * box is loaded as one float4; refused otherwise), as any buffer yn_infer's boxes come from is.  Asynchronous. */
int  yn_slice_append(yn_handle* h, yn_slice* s, int F, const int32_t* shapes_host, int T, const int32_t* tiles_host, int t0, int n,
                     const float* out_boxes_dev, const float* out_scores_dev, const int32_t* out_cls_dev, const int32_t* count_dev, int N,
                     float edge_margin);
/* ONE read-back (list sizes, overflow flag, range mark), per-class NMS of the F lists in yn_nms_merge's arithmetic (never DIoU; kept rows
 * stay in ascending list order) and yn_pack_detections into the object's record buffer.  A range mark returns YN_STATUS_RANGE; a list
 * that would have passed list_capacity fails, naming the first such frame and the rows it needed.  Nothing is delivered then. */
int  yn_slice_merge(yn_handle* h, yn_slice* s, int F, float nms_thresh);
/* The rule yn_slice_merge / yn_slice_infer apply from now on, as yn_merge_rule_tta; expected 0 = 1 (a tile's boxes need no confirmation). */
int  yn_merge_rule_slice(yn_handle* h, yn_slice* s, int rule, int expected);
/* The composition: per chunk of at most the handle's max_batch tiles, in table order, yn_slice_preprocess into the object's input buffer,
 * ONE yn_infer at the handle's current grid and thresholds, one yn_slice_append; then yn_slice_merge.  The grid must be square (its side
 * is the table's `side`); a window grid is refused and nothing is launched.  The result does not depend on where the chunk boundaries
 * fall.  A range mark returns YN_STATUS_RANGE and delivers nothing (acknowledge with yn_range_status, yn_exact_f32(h, 1), run again).
 * F == 0 or T == 0 is an empty result, not an error. */
int  yn_slice_infer(yn_handle* h, yn_slice* s, int F, const uint8_t* const* frames_host, const int32_t* shapes_host, int T,
                    const int32_t* tiles_host, const float* mean_host, const float* std_host, float nms_thresh, float edge_margin);
/* the last successful yn_slice_merge's result, with the contract of yn_tta_result: rec_dev [total][6] + offsets_dev [F+1], owned by the
 * object and valid until its next call.  Any pointer may be NULL; `total` costs one 4-byte read-back (once per result).  Returns 1 when
 * there is no result. */
int  yn_slice_result(yn_slice* s, const float** rec_dev, const int32_t** offsets_dev, int32_t* total);
/* testing aid: the merge lists of the current table (also after a merge that failed on list_capacity), to the host: boxes_host
 * [F][list_capacity][4], scores_host / cls_host [F][list_capacity] (rows >= count: class -1), count_host [F] (the rows the list needed,
 * which may exceed list_capacity) and tile_start_host [T]: where tile t's rows start in its frame's list.  Any pointer may be NULL.
 * Synchronises the stream. */
int  yn_slice_lists(yn_handle* h, yn_slice* s, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host,
                    int32_t* tile_start_host);

/* ---- record lists fused per unit: the third client of the merge lists, for ensembles of models and for fusing any record lists (a TTA
 * result with a sliced one).  max_units 1..4096 lists of list_capacity rows (1..131072); the handle gives the device and the class count. */
typedef struct yn_fuse yn_fuse;
int  yn_fuse_create(yn_handle* h, int max_units, int list_capacity, yn_fuse** out);
void yn_fuse_destroy(yn_fuse* f);
/* empties the B lists */
int  yn_fuse_open(yn_handle* h, yn_fuse* f, int B);
/* rec_dev / offsets_dev in yn_pack_detections' layout for B units: the rows of unit b go to the end of list b in order, the score
 * multiplied by `weight` with one float32 multiply (1.0f copies the bits).  A negative offsets[B] sets the range mark.  A class that is
 * not an integer in 0..C-1 is counted and the next yn_fuse_merge refuses, naming the unit; rows past list_capacity are counted, not
 * written, and the merge refuses on them too.  rec_dev must be 8-byte aligned.  Asynchronous. */
int  yn_fuse_append(yn_handle* h, yn_fuse* f, int B, const float* rec_dev, const int32_t* offsets_dev, float weight);
/* ONE read-back, then the merge of the B lists by `rule` (YN_MERGE_NMS: yn_nms_merge's arithmetic, YN_MERGE_WBF: yn_wbf_merge's) at
 * `thresh`, and yn_pack_detections into the object's record buffer.  expected 0 = the appends since yn_fuse_open.  A range mark returns
 * YN_STATUS_RANGE. */
int  yn_fuse_merge(yn_handle* h, yn_fuse* f, int B, int rule, float thresh, int expected);
/* the last successful yn_fuse_merge's result, with the contract of yn_tta_result */
int  yn_fuse_result(yn_fuse* f, const float** rec_dev, const int32_t** offsets_dev, int32_t* total);
/* testing aid, like yn_slice_lists: boxes_host [B][list_capacity][4], scores_host / cls_host [B][list_capacity], count_host [B].  Any
 * pointer may be NULL.  Synchronises the stream. */
int  yn_fuse_lists(yn_handle* h, yn_fuse* f, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host);

/* How the YN_MERGE_NMS rule of the object suppresses from now on: YN_SOFT_OFF (the default: per-class NMS as before) or a Soft-NMS method
 * with its sigma and score_floor (yn_soft_nms_merge's rule per list; the float argument of yn_tta_infer / yn_slice_merge / yn_slice_infer
 * / yn_fuse_merge stays the IoU threshold).  The setting is kept but unused while the object's rule is YN_MERGE_WBF.  Refused by name: a
 * method outside 0..3, a sigma that is not positive and finite, a score_floor that is negative or not finite. */
int  yn_merge_soft_tta(yn_handle* h, yn_tta* t, int method, float sigma, float score_floor);
int  yn_merge_soft_slice(yn_handle* h, yn_slice* s, int method, float sigma, float score_floor);
int  yn_merge_soft_fuse(yn_handle* h, yn_fuse* f, int method, float sigma, float score_floor);

/* ---- detections painted onto frames in list order: test.py:50-92 / demo.py:48-71 (visualize, plot_bbox_labels) for B frames at once,
 * straight from the rec_dev / offsets_dev pair of yn_pack_detections or yn_tta_result: no read-back, no per-detection host work
 * (DESIGN.md 23 is the specification).  A frame is uint8 [h0][w0][3] BGR on the device, rows contiguous, sides 1..16384.  Records
 * are painted in record order, a later one over an earlier one.  Per record: the box goes to pixels (YN_DRAW_LETTERBOX: the
 * evaluators' bboxes -= offset; /= scale; *= size with geom_host rows w0, h0, rw, rh, left, top, side as yn_eval_add takes them;
 * YN_DRAW_PIXELS: the box is pixels already, only w0, h0 are read), every coordinate through int() (toward zero).  Drawn iff score >
 * vis_thresh (strict, float32); a record that passes this but has a class that is no integer in 0..C-1, a coordinate that is not
 * finite with |v| < 2^30, or '%.2f' digits k = rint(score * 100) outside 0..100 is skipped and counted.  Then, clipped to the frame,
 * inclusive coordinates, a = t / 2, c = (t - 1) / 2: the outline [x1-a, x2+a] x [y1-a, y2+a] minus the hole [x1+c+1, x2-c-1] x
 * [y1+c+1, y2-c-1] (an empty hole: filled) in colors[class]; with labels the title bar [x1, x1 + L*gw + 1] x [y1 - gh - 1, y1] in
 * the same colour, L = strlen(label) + 6, and the text label + ": " + "D.DD", glyph j's cell pixel (r, col) at (x1 + 1 + j*gw + col,
 * y1 - gh + r), black with coverage a8: out = (dst * (255 - a8) + 127) / 255.  The raster rules and the font are this library's own:
 * parity with cv2's rasteriser and Hershey font is not claimed. */
#define YN_DRAW_LETTERBOX 0
#define YN_DRAW_PIXELS    1
typedef struct yn_draw yn_draw;
/* num_classes 1..2000; colors_host [C][3] BGR; labels_host C strings of at most 32 bytes in 32..126, or NULL: outlines only;
 * atlas_host the A8 glyph atlas [95][gh][gw] for ASCII 32..126 with 4 <= gw, gh <= 32, NULL iff labels_host is; thickness 1..8 (the
 * reference: 2).  Everything is copied to the device here. */
int  yn_draw_create(yn_handle* h, int num_classes, const uint8_t* colors_host, const char* const* labels_host, const uint8_t* atlas_host, int gw, int gh,
                    int thickness, yn_draw** out);
void yn_draw_destroy(yn_draw* d);
/* In place, on the handle's stream, asynchronous: frames_host [B] device pointers, geom_host [B][7], rec_dev [rec_capacity][6] (no
 * record at or past rec_capacity is read, whatever the offsets hold), offsets_dev [B+1].  offsets_dev[B] < 0 (the split-f16 range
 * mark) draws nothing and sets the status' range_mark.  Refused before any launch, naming the frame: null pointers, a side outside
 * 1..16384, a bad letterbox geometry, a space that is neither mode, two frames that are the same buffer or overlap; also a handle on another device than the
 * one the object was created on.  B == 0 is not an
 * error.  Work buffers grow with rec_capacity and B (a growth frees the old buffer, which waits for the device). */
int  yn_draw_batch(yn_handle* h, yn_draw* d, int B, uint8_t* const* frames_host, const int32_t* geom_host, int space, const float* rec_dev,
                   const int32_t* offsets_dev, int64_t rec_capacity, float vis_thresh);
/* of the last yn_draw_batch: records drawn, records skipped (see above), range mark.  Any pointer may be NULL.  Synchronises. */
int  yn_draw_status(yn_handle* h, yn_draw* d, int64_t* drawn, int64_t* skipped, int* range_mark);
/* testing aid, like yn_eval_records: the drawn primitives of the last yn_draw_batch in drawing order, host int32 [n][7] = frame,
 * class, x1, y1, x2, y2 (the unclipped integers), k; n = drawn, cap = rows of room.  Synchronises. */
int  yn_draw_prims(yn_handle* h, yn_draw* d, int32_t* host, int64_t cap);

/* ---- detections cut out of frames as fixed-size chips (DESIGN.md 32 is the specification, tests/chip_oracle.py its restatement): the
 * pixels of the detections for a second stage (a classifier, a re-ID embedding, OCR, a zoomed second pass, thumbnails), straight from
 * the rec_dev / offsets_dev pair of yn_pack_detections, yn_tta_result, yn_slice_result, yn_fuse_result or yn_track_update.  Frames,
 * geom_host and space are yn_draw_batch's.  Per record, in record order: selected iff score > min_score (strict, float32) and, after a
 * class that is no integer in 0..C-1 has been skipped and counted, class_keep[class] is set; the box goes to pixels and through int()
 * as for yn_draw_batch (a coordinate that is not finite with |v| < 2^30, or X2 < X1 or Y2 < Y1: skipped); the margin mx = margin_px +
 * (bw0 * margin_permille + 500) / 1000 (my likewise) widens it, the frame clips it (empty, or a side below min_side: skipped); the
 * source rectangle sw x sh is fitted into the cw x ch chip (YN_CHIP_STRETCH: all of it; YN_CHIP_LETTERBOX: Resize.__call__'s arithmetic,
 * sh*cw > sw*ch: rh = ch, rw = (int)((double)sw / sh * ch), left = (cw - rw) / 2; the mirror image; equal: all of it; rw or rh 0:
 * skipped) and resampled like cv2.resize's 8-bit INTER_LINEAR (copy, the exact 2:1 box, or linear: the per-pixel rule of
 * yn_preprocess_batch, the same bits); outside the fitted extent the pixel is fill (BGR).  YN_CHIP_U8: uint8 [slot][ch][cw][3] BGR.
 * YN_CHIP_F32: float32 [slot][3][ch][cw] RGB, every value through Normalize with mean / std (BGR order); with fill[c] = float32(mean[c])
 * * 255 a square letterbox chip is what yn_preprocess_batch writes for the cropped image.  Usable records get the slots 0, 1, 2, ... in
 * record order; those past max_chips are counted as overflow. */
#define YN_CHIP_LETTERBOX 0
#define YN_CHIP_STRETCH   1
#define YN_CHIP_U8  0
#define YN_CHIP_F32 1
typedef struct yn_chip yn_chip;
typedef struct { int32_t cw, ch, fit, format, margin_px, margin_permille, min_side; float min_score, fill[3], mean[3], std[3]; } yn_chip_params;
/* num_classes 1..2000, max_chips 1..65536, cw and ch 8..1024, cw a multiple of 4, margin_px 0..4096, margin_permille 0..4000, min_side
 * 1..16384.  Refused with a reason, in this order: a value outside these limits, a float that is not finite, a std that is not positive,
 * a u8 fill that is no integer in 0..255.  The object has its own lifetime (any handle of its device serves the later calls); its
 * memory shows in yn_live_device_memory. */
int  yn_chip_create(yn_handle* h, int num_classes, const uint8_t* class_keep_host /* [C] or NULL: all */, int max_chips, const yn_chip_params* p, yn_chip** out);
void yn_chip_destroy(yn_chip* c);
/* On the handle's stream, ceil(B / 32) + 2 launches whatever the records hold, no copy back, no synchronise.  B 0..1024; chips_dev
 * [max_chips] chips, 16-byte aligned; index_dev [max_chips] the record index of every slot; rect_dev [max_chips][8] = source x, y, sw,
 * sh, rw, rh, left, top; chip_offsets_dev [B+1]: the slots used by the frames before b, [B] the count.  Slots at or past the count are
 * not written in any output.  No record at or past rec_capacity is read, whatever the offsets hold.  offsets_dev[B] < 0 (the split-f16
 * range mark) is decided on the device: nothing is written but chip_offsets_dev = 0, .., 0, -1, and the status' range word is set.
 * Refused before any launch, in this order: B, rec_capacity or the alignment outside their limits, null pointers, a frame side outside
 * 1..16384 or a bad letterbox geometry (naming the frame), a space that is neither mode, a handle on another device than the object's.
 * B == 0 is no error: chip_offsets_dev[0] = 0 and nothing else.  Work buffers grow with rec_capacity and B (a growth frees the old
 * buffer, which waits for the device). */
int  yn_chip_batch(yn_handle* h, yn_chip* c, int B, const uint8_t* const* frames_host, const int32_t* geom_host, int space,
                   const float* rec_dev, const int32_t* offsets_dev, int64_t rec_capacity,
                   void* chips_dev, int32_t* index_dev, int32_t* rect_dev, int32_t* chip_offsets_dev);
int  yn_chip_status(yn_handle* h, yn_chip* c, int64_t counters_host[4] /* chips, skipped, overflow, range_mark of the last call; synchronises */);

/* ---- detections tracked across video frames: B camera streams, one frame of each per step, identities kept on the device (DESIGN.md 29
 * is the specification, tests/track_oracle.py its float32 restatement; the reference has no tracker, the rules are this library's own,
 * of the ByteTrack / BoT-SORT family with a greedy instead of an optimal assignment).  The input is the rec_dev / offsets_dev pair of
 * yn_pack_detections, yn_tta_result or yn_slice_result; boxes are used in whatever unit they carry.  Per stream max_tracks slots (free,
 * tentative, confirmed, lost), each a constant-velocity Kalman filter in (cx, cy, w, h) with diagonal noise, and an id counter that
 * starts at 1.  One step of one stream: the usable records (finite coordinates, x2 > x1, y2 > y1, score >= track_low; the first
 * max_dets in record order, the rest counted as overflow, the unusable as ignored) -> predict -> IoU -> greedy matching, ties to the
 * lowest slot, then the lowest detection, in three stages (confirmed + lost x high detections at iou_high, confirmed x low at iou_low,
 * tentative x unmatched high at iou_new) -> update / age / free -> births from unmatched high detections with score >= new_thresh into
 * the lowest free slots (none free: dropped_births) -> output.  All decisions in float32, bit-exact with the restatement. */
typedef struct yn_track yn_track;
typedef struct { float track_high, track_low, new_thresh, iou_high, iou_low, iou_new, w_pos, w_vel; int32_t max_lost, min_hits, class_aware; } yn_track_params;
/* streams 1..4096, max_tracks and max_dets 1..128.  p NULL: track_high 0.5, track_low 0.1, new_thresh 0.6, iou_high 0.2, iou_low 0.5,
 * iou_new 0.3, w_pos 1/20, w_vel 1/160, max_lost 30, min_hits 2, class_aware 1.  Refused with a reason: a value that is not finite,
 * track_low > track_high, an IoU threshold outside (0, 1], max_lost < 0, min_hits < 1.  The object has its own lifetime (any handle of
 * its device serves the later calls); its memory shows in yn_live_device_memory. */
int  yn_track_create(yn_handle* h, int streams, int max_tracks, int max_dets, const yn_track_params* p /* NULL: defaults */, yn_track** out);
void yn_track_destroy(yn_track* t);
/* on the handle's stream, asynchronous */
int  yn_track_reset(yn_handle* h, yn_track* t, int stream /* -1: all, and the counters; ids restart at 1 */);
/* B frames; frame b belongs to stream stream_host[b] (NULL: b).  Refused before any launch: B > streams, an index out of range, an index twice, null
 * pointers, a handle on another device.  B == 0 is no error (out_offsets_dev[0] = 0 when the pointer is given, nothing else).  out_rec_dev [B*max_tracks][6] = x1, y1, x2, y2 of the
 * posterior, score, class of every confirmed track matched or born in this step, frame by frame in slot order; out_ids_dev [B*max_tracks]
 * their ids; out_offsets_dev [B+1].  No record at or past rec_capacity is read, whatever the offsets hold (rec_dev may be NULL when it is 0).  offsets_dev[B] < 0 (the
 * split-f16 range mark) is decided on the device: no state word changes, out_offsets_dev = 0, .., 0, -1, one range_mark is counted.  On the
 * handle's stream: ceil(B / 256) + 1 launches, no copy, no synchronise. */
int  yn_track_update(yn_handle* h, yn_track* t, int B, const int32_t* stream_host, const float* rec_dev, const int32_t* offsets_dev, int64_t rec_capacity,
                     float* out_rec_dev, int32_t* out_ids_dev, int32_t* out_offsets_dev);
/* testing aids; both synchronise.  A free slot reads 0, 0, 0, 0, -1 and zeros.  Any pointer of yn_track_state may be NULL. */
int  yn_track_state(yn_handle* h, yn_track* t, int stream, int32_t* meta_host /* [max_tracks][5] state (0 free, 1 tentative, 2 confirmed, 3 lost), id, hits, lost_age, detection matched or born from in the last step or -1 */,
                    float* filt_host /* [max_tracks][22] class, score, then p, v, P00, P01, P11 for cx, cy, w, h */, int32_t* next_id);
int  yn_track_status(yn_handle* h, yn_track* t, int64_t counters_host[6] /* steps (frames stepped), births, dropped_births, overflow, ignored, range_marks; summed since create / reset(-1) */);

/* ---- training loss (train.py:219-229, forward value + gradient w.r.t. the raw predictions) ---------- */
/* models/yolo_nano.py:332-358 + tools.iou_score (tools.py:219-233) + tools.loss (tools.py:236-276).
 * Predictions in the reference's split layout: conf [B,N] (= [B,N,1]), cls [B,N,C], txtytwth [B,N,4];
 * target [B,N,11] = [obj, cls, tx,ty,tw,th, weight, x1,y1,x2,y2] as tools.multi_gt_creator builds it (tools.py:108).
 * losses_dev[4] = conf, cls, bbox (txty+twth), iou — each already divided by B.  The three gradient buffers
 * (same shapes as the predictions; all or none) receive d(conf+cls+bbox+iou)/d(prediction), i.e. what
 * `total_loss.backward()` (train.py:222-229) leaves in the prediction tensors; gt_conf = iou.detach(). */
int  yn_loss(yn_handle* h, const float* conf_dev, const float* cls_dev, const float* txtytwth_dev,
             const float* target_dev, int B, float* losses_dev,
             float* g_conf_dev, float* g_cls_dev, float* g_txtytwth_dev);
/* Same, reading the predictions from / writing the gradients to the three raw NHWC head tensors
 * (layout of yn_forward_raw), i.e. without the re-layout copies of models/yolo_nano.py:308-330. */
int  yn_loss_heads(yn_handle* h, const float* head_s8_dev, const float* head_s16_dev, const float* head_s32_dev,
                   const float* target_dev, int B, float* losses_dev,
                   float* g_s8_dev, float* g_s16_dev, float* g_s32_dev);

/* torch.optim.SGD(lr, momentum=0.9, weight_decay=5e-4).step() (train.py:167-171, 230) on ONE flat float32 bucket
 * holding every parameter (1.27-1.33 M elements), fused with the 1/world_size averaging of the all-reduced
 * gradient sum:  g = grads*grad_scale + wd*p ; buf = first_step ? g : momentum*buf + g ; p -= lr*buf.
 * A bucket that holds a NaN or Inf leaves parameters and momentum untouched — the reference skips an iteration whose loss is
 * NaN (train.py:225-226); after the data-parallel all-reduce every rank sees the same non-finite bucket, so all ranks skip
 * together without a host round trip (every finite gradient, +-FLT_MAX included, is a step).  n = 0 does nothing.
 * yn_train_skipped_steps reads the number of skipped updates (synchronises). */
int  yn_sgd_step(yn_handle* h, float* params_dev, const float* grads_dev, float* momentum_buf_dev, int64_t n,
                 float lr, float momentum, float weight_decay, float grad_scale, int first_step);

/* ---- ModelEMA.update (utils/misc.py:76-86): ema[i] = ema[i] * d + (1 - d) * model[i] over one float32 tensor (or one flat
 * buffer), d = decay * (1 - exp(-updates / 2000)) computed by the caller in double like the reference; the kernel keeps
 * torch's rounding sequence, so the result is bit-identical to the reference's in-place update. */
int  yn_ema_update(yn_handle* h, float* ema_dev, const float* model_dev, int64_t n, double decay);

/* ---- training labels: tools.multi_gt_creator (tools.py:97-216, call site train.py:212) --------------------------------
 * labels_dev float64 [total][5] = xmin, ymin, xmax, ymax (fractions of the image), class — the objects of image b are rows
 * offsets_dev[b] .. offsets_dev[b+1]-1 IN LIST ORDER (a later object overwrites the slot of an earlier one, as in the
 * reference).  anchors_host: the 9 [w,h] pairs in input pixels as float64 (the reference's Python floats; the float32
 * copy inside the handle would move IoU ties).  target_dev float32 [B][N][11] = obj, cls, tx, ty, tw, th, weight,
 * xmin, ymin, xmax, ymax is fully overwritten.  N and the grid come from the handle's current input size. */
int  yn_make_targets(yn_handle* h, const double* labels_dev, const int32_t* offsets_dev, int B, const double* anchors_host, float* target_dev);

/* ---- training step (train.py:212-231) ---------------------------------------------------------------- */
/* Parameters, gradients and SGD momentum live in three caller-owned FLAT float32 device buffers of
 * yn_train_param_count() elements, in nn.Module.named_parameters() order of the reference model (per layer:
 * conv.weight, [conv.bias], [bn.weight, bn.bias]); yn_train_param_offset maps a state-dict key to its slice.
 * yn_train_bind copies the loaded state dict into `params`, zeroes `grads` / `momentum`.  BatchNorm running statistics
 * stay inside the handle (updated in place, momentum 0.1; read back with yn_read_param). */
int64_t yn_train_param_count(yn_handle* h);
int  yn_train_param_offset(yn_handle* h, const char* state_dict_key, int64_t* offset, int64_t* numel);
int  yn_train_bind(yn_handle* h, float* params_dev, float* grads_dev, float* momentum_dev, int64_t n);
/* One step: train-mode forward (BatchNorm batch statistics) of x [B,3,S,S], the four losses of tools.loss against
 * target [B,N,11] into losses_dev[4], backward into `grads` (overwritten).  do_update != 0 also applies
 * SGD(lr, momentum, weight_decay) with grads*grad_scale; data-parallel callers pass do_update = 0, all-reduce `grads`
 * (RCCL, one flat bucket) and then call yn_sgd_step(grad_scale = 1/world).  Call yn_fold_bn before the next inference. */
int  yn_train_step(yn_handle* h, const float* x_dev, const float* target_dev, int B, float lr, float momentum,
                   float weight_decay, float grad_scale, int do_update, float* losses_dev);
int  yn_read_param(yn_handle* h, const char* state_dict_key, float* host, int64_t numel);
/* The fp16 step's dynamic loss scale (initial 1024; halved on an overflowing step, doubled after 2000 clean ones; all on the device).
 * The decision is taken by yn_sgd_step from the finite-scan of the bucket it applies - after the data-parallel all-reduce that bucket is
 * the same on every rank, so the replicas' scales move together.  get / set (both synchronise) let a checkpoint carry the scale and its
 * clean-step counter across a resume; set before the first fp16 step replaces the default start value.  set also discards the overflow
 * flag / pending mark of a step that has not been settled yet (the restored state starts clean).  Accepted range [1, 2^30]; the device
 * only ever DOUBLES up to 65536, so a larger restored value can only shrink. */
int  yn_train_get_loss_scale(yn_handle* h, float* scale, float* clean_steps);
int  yn_train_set_loss_scale(yn_handle* h, float scale, float clean_steps);
/* The gradient exchange of the data-parallel step (train.py:13-14 imports DistributedDataParallel; BASELINE configs[2]: "DDP grad
 * all-reduce over xGMI") for callers WITHOUT torch: all-reduce(sum), in place, of the bound flat gradient buffer over an RCCL
 * communicator the caller owns (`nccl_comm` is an ncclComm_t), enqueued on the handle's stream — after yn_train_step(do_update = 0),
 * before yn_sgd_step(grad_scale = 1/world).  One 5.3 MB bucket per step: no bucketing, no overlap needed at this model size.
 * The library does not link RCCL: ncclAllReduce is resolved at run time from the librccl already loaded in the process (the one
 * that created the communicator), else from librccl.so.1.  torch users keep torch.distributed (parallel.dp_train_step). */
int  yn_allreduce_grads(yn_handle* h, void* nccl_comm);
/* The forward half of yn_train_step on its own — `model.train(); model.backbone/neck/heads(x)` (models/yolo_nano.py:284-301 with
 * BatchNorm batch statistics; the running statistics ARE updated) in the precision selected by yn_train_precision: the three
 * raw NHWC head tensors as dense float32 [B,S/8,S/8,A(5+C)], [B,S/16,..], [B,S/32,..].  Parity hook for the train-mode network. */
int  yn_train_forward(yn_handle* h, const float* x_dev, int B, float* head_s8_dev, float* head_s16_dev, float* head_s32_dev);
int  yn_train_skipped_steps(yn_handle* h, int64_t* count_host);
/* The fp16 step forks the head towers of levels 3 / 4 onto streams of their own when that measured faster on this device (a handle's
 * steps 3-6 time the step both ways, so the choice - and with it the order of some atomic sums - depends on the machine).  Query the
 * decision (force = 0; *decision: -1 undecided, 0 one stream, 1 forked) or pin it for reproducible runs (force = 1: one stream, 2: forked). */
int  yn_train_head_fork(yn_handle* h, int force, int* decision_host);
/* Arithmetic of yn_train_step (BASELINE configs[2] names fp16; train.py itself runs fp32).  YN_F32 (default): fp32 end to end.
 * YN_F16: activations and activation gradients are STORED as fp16 (channel-padded NHWC, half the HBM bytes), every GEMM-shaped
 * conv (forward, input gradient, weight gradient) runs on the f16 MFMA with fp32 accumulation, BatchNorm statistics / parameter
 * gradients / the optimiser stay fp32 on the fp32 master weights, and the loss gradient is multiplied by a dynamic loss scale
 * kept on the device (halved when a step's gradients overflow — that step is skipped — doubled after 2000 clean steps).
 * YN_F16 is refused, with a message, for a network with a BatchNorm, depthwise or biased layer above 256 padded channels (the 1.5x and
 * 2.0x backbones: bf = 352 / 488): the step's reducing and BatchNorm kernels combine at most 32 channel octets.  Those train in fp32. */
int  yn_train_precision(yn_handle* h, int dtype);
/* Opt-in: the fp16 step replays everything between its host-side preparation and the optimiser (~540 launches on two streams) from a
 * hipGraph once the same (x, target, batch, grid) has been seen twice on a handle with a stream of its own; callers whose tensors'
 * addresses never repeat stay on direct launches.  Off by default: measured slower than direct launches on this runtime.
 * enable: 1 / 0 switch it, -1 leaves it; replays (optional) receives the number of steps served from a graph so far. */
int  yn_train_graph(yn_handle* h, int enable, int64_t* replays);

/* ---- single operators (op-level parity tests; NHWC float32 device tensors) ------------------ */
/* weights in the reference (torch) layout on the DEVICE: dw [C,1,3,3], pw [Cout,Cin,1,1],
 * dense [Cout,Cin,3,3]; bias [Cout] or NULL. */
int  yn_op_dwconv3x3(yn_handle* h, const float* x, int B, int H, int W, int C, int stride,
                     const float* w, const float* bias, int act, float* y);
int  yn_op_pwconv(yn_handle* h, const float* x, int B, int H, int W, int Cin, int Cout,
                  const float* w, const float* bias, int act, float* y);
/* Up to three pointwise convs as ONE grouped launch, as the network runs the three FPN laterals (models/yolo_nano.py:286-296): member p
 * reads M[p] rows of Cin[p] floats at x[p] + m * in_ld[p] + in_off[p] and writes Cout floats at y[p] + m * out_ld[p] + out_off[p], on the
 * caller's tensors.  Cin, in_ld and in_off even.  The kernel is the handle's choice (autotuner, or yn_set_pw_config: every index of the
 * split-f16 family gives the same bits; the last one is pw_pipe_group_kernel where it has a form for the members). */
int  yn_op_pwconv_group(yn_handle* h, int n, const float* const* x, const int* in_ld, const int* in_off, const int* M, const int* Cin, int Cout,
                        const float* const* w, const float* const* bias, int act, float* const* y, const int* out_ld, const int* out_off);
/* The tail of a ShuffleV2Block (backbone/shufflenetv2.py:72,74 + channel_shuffle :14-28) exactly as the network runs it:
 * y = channel_shuffle(cat(pass, act(pw(x))), 2), i.e. y[..., 2j] = pass[..., j], y[..., 2j+1] = act(pw(x))[..., j], written by
 * the GEMM epilogue (the shuffle is never materialised on its own).  pass [B,H,W,Cout], y [B,H,W,2*Cout]. */
int  yn_op_pwconv_shuffle(yn_handle* h, const float* x, const float* pass, int B, int H, int W, int Cin, int Cout,
                          const float* w, const float* bias, int act, float* y);
/* x2/resample: 0 none, 1 add nearest-up2 of x2 [B,H/2,W/2,Cin], 2 add nearest-down of x2 [B,2H,2W,Cin]
 * (models/yolo_nano.py:291-296 fused into the conv's prologue).  Cin must be a multiple of 32. */
int  yn_op_conv3x3(yn_handle* h, const float* x, const float* x2, int resample, int B, int H, int W,
                   int Cin, int Cout, const float* w, const float* bias, int act, float* y);
/* stem: x NCHW [B,3,H,W] -> y NHWC [B,Ho,Wo,Cout], 3x3 stride 2 pad 1 (backbone/shufflenetv2.py:109) */
int  yn_op_stem(yn_handle* h, const float* x_nchw, int B, int H, int W, int Cout,
                const float* w, const float* bias, int act, float* y);
/* the stem as the network runs it: conv + activation + max pool 3x3 stride 2 pad 1 in one kernel (stem_pool_kernel),
 * x NCHW [B,3,H,W] -> y NHWC [B,Hp,Wp,Cout], Hp = ((H-1)/2+1 - 1)/2 + 1 */
int  yn_op_stem_pool(yn_handle* h, const float* x_nchw, int B, int H, int W, int Cout,
                     const float* w, const float* bias, int act, float* y);
int  yn_op_maxpool3x3s2(yn_handle* h, const float* x, int B, int H, int W, int C, float* y);
/* ShuffleV2Block (backbone/shufflenetv2.py:31-78), weights taken from the handle's loaded params:
 * block = "backbone.stage2.1" etc.  x [B,H,W,Cin] -> y [B,H/stride,W/stride,Cout]. */
int  yn_op_shuffle_block(yn_handle* h, const char* block, const float* x, int B, int H, int W, float* y);
/* A stride-2 ShuffleV2Block as the ONE kernel yn_down_fuse selects inside the network (stage 2 of 1.0x / 0.5x), on any even map:
 * x [B,H,W,Cin] -> y [B,H/2,W/2,Cout].  Split-f16 family; independent of yn_down_fuse and yn_set_pw_config.  An error where that kernel
 * does not cover the block or the handle is on the exact-f32 family: yn_op_shuffle_block is the five-launch form. */
int  yn_op_down_unit(yn_handle* h, const char* block, const float* x, int B, int H, int W, float* y);
/* The candidate decode on its own (models/yolo_nano.py:308-330, 120-156, 362-367, 253-261): dense raw NHWC heads with row stride A(5+C),
 * as for yn_score_full -> boxes [B,N,4] (normalised, clamped), best score [B,N], class [B,N] int32 (-1 where score < conf_thresh; a
 * candidate of a wavefront that is below the threshold by objectness alone has score 0).  decode_kernel<false, KMAX>, KMAX by C. */
int  yn_op_decode_cand(yn_handle* h, const float* head_s8, const float* head_s16, const float* head_s32, int B, float conf_thresh,
                       float* boxes, float* scores, int32_t* cls);
/* yn_infer's forward from the output of the heads' layer .1 to the candidate arrays, on caller-provided activations x8 [B,S/8,S/8,96],
 * x16, x32 (NHWC): layers .2, .3, .4 with the handle's loaded, folded weights and the decode, through the kernels the handle's current
 * yn_tail_fuse / yn_fuse_decode / yn_group_launch switches and conf_thresh select (the same function yn_infer calls; the profile
 * records name the kernels).  Outputs as yn_op_decode_cand.  Synchronises the stream. */
int  yn_op_head_tail(yn_handle* h, const float* x8, const float* x16, const float* x32, int B, float* boxes, float* scores, int32_t* cls);
/* NCHW <-> NHWC helpers for the tests and the host shim */
int  yn_op_nchw_to_nhwc(yn_handle* h, const float* x, int B, int C, int H, int W, float* y);
int  yn_op_nhwc_to_nchw(yn_handle* h, const float* x, int B, int C, int H, int W, float* y);

/* Single kernels of the fp16 training step (yn_train_precision YN_F16) behind fp32 NHWC device tensors, for op-level parity: the
 * inputs are rounded to fp16 into the step's channel-padded layout (gapped != 0: the two-plane layout of a ShuffleV2 unit output,
 * Cin = 2*bf), ONE kernel per requested result runs, the fp16 results return as fp32.  kind 0 pointwise, 1 depthwise 3x3
 * (stride 1|2), 2 dense 3x3; w / dw in the reference layouts; y = conv(x) + bias, dx / dw = the gradients for dy (null = skip). */
int  yn_op_h16_conv(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, const float* w, const float* bias,
                    int Cout, int stride, const float* dy, float* y, float* dx, float* dw);
/* yn_op_h16_conv with the argument forms the step itself uses.  Every launch under test runs inside a profile bracket of its own
 * (yn_profile_enable: the records then name the kernels that ran, in order: forward, dx, dbias, dw, the combine).
 *   x [B,H,W,x_ld], channels [x_off, x_off + Cin): the whole row (x_ld = Cin, x_off = 0), or one plane of an ungapped two-plane unit
 *   tensor (x_ld = 2 Cin, x_off = 0 | Cin: staged as [x1 | pad][x2 | pad], the conv reads its plane in place); other slices are refused.
 *   dx [B,H,W,dx_ld], in and out, same two forms: its contents are staged first, the input gradient is written (accumulate != 0: added)
 *   into the conv's channels and the whole tensor comes back (fp16-rounded).
 *   partial_cap: floats of weight-gradient scratch the launcher may use (0 = the entry's 4 Mi; at least one packed copy of dw).
 *   dbias [Cout]: column sums of dy through hcol_reduce_kernel<3> into the gradient slots; dw and dbias are combined from the slots by
 *   hgrad_finish_kernel (S = 1) as at the end of a step.  dw of a depthwise conv and dbias need at most 256 padded channels.
 *   stat (depthwise stride 1, at most 256 padded channels): 1 = sums_fwd[0][c] = sum y, [1][c] = sum y^2 of the stored fp16 output;
 *   2 = with the complete dense dx, sums_bwd as yn_op_h16_gemm_stats (y_below [B,H,W,Cin] in x's channel map).  Host double [2][Cin]. */
int  yn_op_h16_conv2(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, int x_ld, int x_off,
                     const float* w, const float* bias, int Cout, int stride, const float* dy, int accumulate, int dx_ld, int dx_off,
                     int64_t partial_cap, int stat, const float* y_below, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, int act, float* y, float* dx, float* dw, float* dbias, double* sums_fwd, double* sums_bwd);
/* The fp16 step's stem conv (3 -> 24, 3x3 stride 2 pad 1) over x [B,3,H,W] fp32 NCHW: y [B,Ho,Wo,24] (null = skip); with dy also
 * dw [24][3][3][3] = hstem_wgrad_kernel's sums in zeroed gradient slots, combined by hgrad_finish_kernel (S = 1).  bias [24] or null. */
int  yn_op_h16_stem(yn_handle* h, const float* x_nchw, int B, int H, int W, const float* w, const float* bias, const float* dy, float* y, float* dw);
/* The fp16 step's 3x3 stride-2 max pool over x [B,H,W,C] (C a multiple of 8): y, idx [B,Ho,Wo,C] (one byte per element: the window
 * position ky * 3 + kx of the first maximum in scan order); with dy also dx [B,H,W,C]. */
int  yn_op_h16_maxpool(yn_handle* h, const float* x, int B, int H, int W, int C, const float* dy, float* y, uint8_t* idx, float* dx);
/* The stem's BatchNorm + activation + max pool as the fp16 step fuses them, from the stem conv's output y [B,H,W,24]: statistics
 * (hcol_reduce_kernel<0>), then hstem_apply_pool_kernel -> out, idx [B,Ho,Wo,24] (as yn_op_h16_maxpool), mean, invstd [24] (device);
 * with the pooled tensor's gradient g1 [B,Ho,Wo,24]: hstem_bwd_kernel<0> and <1> -> dy [B,H,W,24], dgamma, dbeta [24]. */
int  yn_op_h16_stem_pool(yn_handle* h, const float* y, int B, int H, int W, const float* gamma, const float* beta, int act, const float* g1,
                         float* out, uint8_t* idx, float* mean, float* invstd, float* dy, float* dgamma, float* dbeta);
/* hresample_kernel: the modes of yn_op_f32_resample on fp16 tensors (modes 2 / 3 add into the prior contents of out; H, W even for
 * modes 0 / 2). */
int  yn_op_h16_resample(yn_handle* h, int mode, const float* a, const float* b, float* out, int B, int H, int W, int C);
/* hgather_kernel with every map argument of launch_hgather: dst[m][dp(j)] = src[m][sp(j)] for j < n, 0 for n <= j < npad, where
 * sp(j) = l + (l >= src_half ? src_gap : 0), l = src_off + j * src_cs (dp alike).  src [M][src_ld] and dst [M][dst_ld] (in and out)
 * are PHYSICAL rows, pads included.  A map that leaves a row is refused. */
int  yn_op_h16_gather(yn_handle* h, const float* src, int src_ld, int src_off, int src_cs, int src_half, int src_gap,
                      float* dst, int dst_ld, int dst_off, int dst_cs, int dst_half, int dst_gap, int64_t M, int n, int npad);
/* The end of an fp16 backward pass: hgrad_finish_kernel (g[n] = (g + the 8 slot copies slots[8][n]) / S, overflow scan), then
 * hscale_update_kernel (update 0: not run; 1: settles from the local flag; 2: from global_flag, as yn_sgd_step passes its
 * bucket-wide one).  state: five 32-bit words on the HOST, in and out: S, 1 / S, clean steps, the overflow flag (an integer), pending. */
int  yn_op_h16_grad_finish(yn_handle* h, float* g, const float* slots, int64_t n, float* state, int update, int global_flag);
/* The fp16 step's loss on its own (loss_kernel<true, fp16> + loss_reduce_kernel): the three dense fp32 raw heads [B,S/s,S/s,A(5+C)] are
 * rounded to fp16 rows of the step's physical width (A(5+C) rounded up to a multiple of 8: 80 for VOC's 75, 256 for COCO's 255), the
 * gradient rows are zeroed as the step zeroes them, `scale` (> 0) is the loss scale of a state block of this call's own.  losses [4]
 * (device, fp32); g_* (device, all three or none): the head gradients * scale as the kernel stored them in fp16, dense fp32;
 * pad_nonzero (host, may be null): how many elements of the gradient rows' pad columns are not +0. */
int  yn_op_h16_loss(yn_handle* h, const float* head_s8, const float* head_s16, const float* head_s32, const float* target, int B, float scale,
                    float* losses, float* g_s8, float* g_s16, float* g_s32, int* pad_nonzero);
/* The column sums the fp16 step takes in its GEMM epilogues instead of separate reduction launches, on their own (kind 0 pointwise,
 * 2 dense 3x3; layouts as yn_op_h16_conv): y = conv(x) with sums_fwd[0][c] = sum y, sums_fwd[1][c] = sum y^2 over the STORED fp16
 * values (the train-mode BatchNorm statistics, utils/modules.py:12-21);  and, when dy is given, dx = the input gradient with
 * sums_bwd[0][c] = sum d, sums_bwd[1][c] = sum d * xhat, d = dx * act'(BN(y_below)), xhat = (y_below - mean) * invstd — the two sums
 * the BatchNorm backward of the layer BELOW needs (y_below [B,H,W,Cin] its pre-BN output; mean / invstd / gamma / beta [Cin] device
 * pointers).  sums are host double [2][channels]. */
int  yn_op_h16_gemm_stats(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int gapped, const float* w, int Cout,
                          float* y, double* sums_fwd, const float* dy, const float* y_below, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, int act, float* dx, double* sums_bwd);
/* Train-mode BatchNorm (+ activation) forward over y [M][C] and, when dz is given, its backward: z, dy [M][C], dgamma, dbeta [C].
 * yn_op_h16_bn2 also returns the saved statistics mean, invstd [C] (device; null = skip).  C <= 256. */
int  yn_op_h16_bn(yn_handle* h, const float* y, const float* dz, int64_t M, int C, const float* gamma, const float* beta, int act,
                  float* z, float* dy, float* dgamma, float* dbeta);
int  yn_op_h16_bn2(yn_handle* h, const float* y, const float* dz, int64_t M, int C, const float* gamma, const float* beta, int act,
                   float* z, float* dy, float* dgamma, float* dbeta, float* mean, float* invstd);
/* The same BatchNorm as the last layer of a ShuffleV2 unit (backbone/shufflenetv2.py:69-78 with :14-28): forward writes the unit
 * output unit[m][2c] = pass[m][c], unit[m][2c+1] = act(BN(y))[m][c]  ([M][2C]: concat + channel_shuffle(2));  backward takes the unit
 * output's gradient dunit [M][2C] and returns dy [M][C] (through activation and BatchNorm), deven [M][C] = dunit[:, 0::2] (the
 * pass-through half, written by the backward kernel on its way: it loads those values anyway), dgamma, dbeta [C].  C <= 128. */
int  yn_op_h16_bn_unit(yn_handle* h, const float* y, const float* pass, const float* dunit, int64_t M, int C, const float* gamma, const float* beta,
                       int act, float* unit, float* dy, float* deven, float* dgamma, float* dbeta);

/* Single layers of the fp32 training step (the default precision) over fp32 device tensors, for op-level tests against a float64
 * reference.  Each entry runs the step's own per-layer launch code: the same weight packs, tile / kernel choices, weight-gradient
 * scratch, gradient slots (+ their combine) and BatchNorm double accumulators as yn_train_step.
 * One conv: kind 0 pointwise, 1 depthwise 3x3 (stride 1|2), 2 dense 3x3, 3 stem (3 -> 24, stride 2).  x is NHWC [B*H*W][x_ld] and the
 * conv reads its channels [x_off, x_off + Cin) (a channel slice of a wider tensor, as the second half of a ShuffleV2 unit tensor);
 * the stem takes NCHW [B,3,H,W] with x_ld = x_off = 0.  w / dw in the reference layouts.  y = conv(x) + bias, [B*Ho*Wo][y_ld]; y_ld =
 * Cout, or for a pointwise conv Cout rounded up to a multiple of 4 (the row padding of a BN-less head conv: the extra columns of y are
 * written as zeros, those of dy must be zeros).  For dy [B*Ho*Wo][y_ld] any of dx (the geometry of x: only the conv's channels are
 * touched; accumulate != 0 adds to what is there), dw and dbias [Cout] is computed (null = skip; the stem has no dx).
 * partial_cap: floats of weight-gradient scratch, 0 = as much as the step has (a small value forces the launchers to clip their slice count). */
int  yn_op_f32_conv(yn_handle* h, int kind, const float* x, int B, int H, int W, int Cin, int x_ld, int x_off, const float* w, const float* bias,
                    int Cout, int stride, int y_ld, int64_t partial_cap, const float* dy, int accumulate, float* y, float* dx, float* dw,
                    float* dbias);
/* Train-mode BatchNorm (+ activation) over y [M][C], C even, as nn.BatchNorm2d(momentum = 0.1, eps = 1e-5).train() (utils/modules.py:12-21): z,
 * the batch mean and 1 / sqrt(biased variance + eps) [C], running_mean / running_var [C] updated in place (unbiased variance; both null =
 * skip).  unit == 0: z [M][C]; with dz, a view of rows dz_ld whose channels start at dz_off, also dy [M][C], dgamma, dbeta [C].
 * unit != 0, the last layer of a ShuffleV2 unit (backbone/shufflenetv2.py:69-78 with :14-28): z is the unit output [M][2C] with
 * z[m][2c] = pass[m][c] (pass [M][C]) and z[m][2c+1] = act(BN(y))[m][c]; dz is the unit output's gradient [M][2C] (dz_ld / dz_off
 * unused), read at its odd channels; deven [M][C] = dz[:, 0::2], the pass-through half. */
int  yn_op_f32_bn(yn_handle* h, const float* y, int64_t M, int C, const float* gamma, const float* beta, int act, int unit, const float* pass,
                  float* running_mean, float* running_var, float* z, float* mean, float* invstd, const float* dz, int dz_ld, int dz_off,
                  float* dy, float* deven, float* dgamma, float* dbeta);
/* 3x3 stride-2 max pool (pad 1) that records its arg-max: y, idx [B,Ho,Wo,C] (idx = iy*W + ix of the first maximum in window scan
 * order, as F.max_pool2d(return_indices=True)); with dy also dx [B,H,W,C] (C even). */
int  yn_op_f32_maxpool(yn_handle* h, const float* x, int B, int H, int W, int C, float* y, int32_t* idx, const float* dy, float* dx);
/* The FPN / PAN adds (models/yolo_nano.py:291-296) and their backwards, every tensor NHWC with C channels:
 * mode 0  out[B,H,W] = a[B,H,W] + up2(b[B,H/2,W/2])          mode 1  out[B,H,W] = a[B,H,W] + b[B,2H,2W] at the even pixels
 * mode 2  out[B,H/2,W/2] += the four children of a[B,H,W]     mode 3  out[B,2H,2W] at the even pixels += a[B,H,W]          (b unused) */
int  yn_op_f32_resample(yn_handle* h, int mode, const float* a, const float* b, float* out, int B, int H, int W, int C);

/* ---- baseline JPEG decode: Huffman stage on the host, everything after it on the device --------------------------------------------
 * Files as cv2.imread / PIL read them with libjpeg's defaults (JDCT_ISLOW, fancy upsampling), byte for byte: SOF0 / SOF1 with 8-bit
 * samples, one interleaved scan, 1 component or 3 with luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma, restart intervals, 8- and 16-bit
 * quantisation tables.  Anything else (progressive, arithmetic, lossless, 12-bit, 4 components, other samplings, several scans) is
 * YN_JPEG_UNSUPPORTED; a file that breaks its own syntax (truncated, codes outside a table, runs past coefficient 63, bad restart markers,
 * undefined tables, a dimension of 0) is YN_JPEG_CORRUPT; a side above 16384, or a coefficient buffer that is too small, YN_JPEG_TOO_LARGE. */
typedef struct yn_jpeg yn_jpeg;
#define YN_JPEG_OK 0
#define YN_JPEG_UNSUPPORTED 1
#define YN_JPEG_CORRUPT 2
#define YN_JPEG_TOO_LARGE 3
/* Host only, no handle, no GPU needed.  info8 = w, h, components, h_samp, v_samp (of the luma), restart interval, SOF marker, status.
 * Returns the status. */
int  yn_jpeg_info(const uint8_t* data, int64_t len, int32_t* info8);
/* Host only: the entropy stage alone.  coef_host [cap] int16 receives the coefficients, 64 per block in natural order, per component
 * block-row-major over the MCU-padded block grid, component after component; qt_host [3][64] the components' quantisation tables in
 * natural order; grid_host [3][2] the block grids (blocks high, blocks wide; 0 for absent components).  Returns the status, also in *status. */
int  yn_jpeg_coefficients(const uint8_t* data, int64_t len, int16_t* coef_host, int64_t cap, uint16_t* qt_host, int32_t* grid_host, int32_t* status);
/* A decoder for the handle's device: two pinned staging slots of staging_bytes each (int16 coefficients: 2 bytes per sample, 3 bytes
 * per pixel at 4:2:0), 1.5 x staging_bytes on the device.  A batch is cut into chunks of max_batch (1..1024) images, one upload and two
 * kernel launches each; the host decodes a chunk with up to `threads` (>= 1, capped at 16) workers. */
int  yn_jpeg_create(yn_handle* h, int max_batch, int64_t staging_bytes, int threads, yn_jpeg** out);
void yn_jpeg_destroy(yn_jpeg* j);
/* n files (host pointers / lengths) -> frames_host[i]: a DEVICE pointer to uint8 [h_i][w_i][3] BGR, sized by yn_jpeg_info.  Returns once
 * the work is enqueued on the handle's stream (the entropy stage has run by then: the files may be released).  status_host[i] is the
 * YN_JPEG_ status of image i and *failed the number that are not OK: such a frame is left untouched (and may be null), the others are
 * decoded.  A chunk whose coefficients exceed staging_bytes fails the call (1) before anything is launched; the error names the bytes needed. */
int  yn_jpeg_decode_batch(yn_handle* h, yn_jpeg* j, int n, const uint8_t* const* data_host, const int64_t* len_host, uint8_t* const* frames_host,
                          int32_t* status_host, int32_t* failed);
/* Why image i of the last batch was refused ("" if it was not).  j == NULL: the reason of the calling thread's last yn_jpeg_info /
 * yn_jpeg_coefficients. */
const char* yn_jpeg_reason(yn_jpeg* j, int i);
/* Measurement (synchronises): ms3 = host entropy stage of the last batch (wall clock), upload and kernels of its last chunk (HIP events).
 * In entropy mode 1 the host time is the copy pass plus any files the host decoded after all, and the upload time runs from the first
 * upload to the last, the entropy kernels in between included (yn_jpeg_entropy_timing splits them). */
int  yn_jpeg_timing(yn_handle* h, yn_jpeg* j, float* ms3);
/* ---- the entropy mode of a decoder: the Huffman stage on the host (default) or on the device (opt-in) ---------------------------------------
 * mode 0: the host decodes, as described above.  mode 1: the host only parses the markers and copies each scan once (byte stuffing and
 * restart markers go); the device decodes it in subsequences of subseq_bits (a multiple of 32; 0 = the default, 1024) that synchronise in
 * at most max_rounds rounds (0 = the default, 64), and hands the same coefficients to the same kernels.  A file the device cannot vouch for
 * (no fixed point within max_rounds, anything entropy_decode would refuse, block counts that disagree with the header, restart markers
 * out of order) is decoded by the host after all, so frames, statuses and reasons are those of mode 0 in every case.  In mode 1
 * yn_jpeg_decode_batch waits, per chunk, for one result word per file before it enqueues the pixel kernels; the scans are staged in a
 * further slot pair of staging_bytes (a chunk whose scans exceed it fails the call like one whose coefficients do).  Setting a mode
 * synchronises the device and resets the statistics.  Returns 1 for values out of range; the reason is yn_jpeg_reason(NULL, 0). */
int  yn_jpeg_entropy(yn_jpeg* j, int mode, int subseq_bits, int max_rounds);
/* Since the mode was set: files whose coefficients the device decoded, files that took the host decoder in mode 1; of the last chunk: the
 * largest number of rounds a file used and the number of subsequences.  All 0 in mode 0. */
int  yn_jpeg_entropy_stats(yn_jpeg* j, int64_t* device_files, int64_t* host_files, int32_t* rounds_last, int32_t* subseqs_last);
/* Testing aid (synchronises): the coefficients of file i of the last chunk as the device's entropy stage left them, in exactly
 * yn_jpeg_coefficients' layout.  Fails for a file that took the host decoder: the device wrote none for it. */
int  yn_jpeg_device_coefficients(yn_handle* h, yn_jpeg* j, int i, int16_t* host, int64_t cap);
/* Testing aid (synchronises): per subsequence of file i of the last chunk the state its decode started from at the fixed point and the
 * blocks finished before it: host [subsequences][4] = bit position in the unstuffed scan, unit in the MCU, zigzag index, blocks before.
 * cap counts int32 elements; the error names the number needed. */
int  yn_jpeg_entropy_states(yn_handle* h, yn_jpeg* j, int i, int32_t* host, int64_t cap);
/* Host only, no handle, no GPU: the copy pass of mode 1 for one file.  unstuffed_host [cap] receives the scan without byte stuffing and
 * restart markers (cap >= len always suffices), segments_host [seg_cap][2] = first byte in it and first MCU of every restart segment,
 * info4 = unstuffed bytes, segments found, 1 if the file must take the host decoder (markers damaged or misnumbered, a segment count that
 * disagrees with the header), segments the header asks for.  Returns the parser's status, YN_JPEG_TOO_LARGE when a buffer is too small. */
int  yn_jpeg_scan_prepare(const uint8_t* data, int64_t len, uint8_t* unstuffed_host, int64_t cap, int32_t* segments_host, int64_t seg_cap, int32_t* info4);
/* Measurement (synchronises): of the last chunk decoded in mode 1, HIP event times in ms: upload of scans and tables, clearing the
 * coefficients, jpeg_huff_first_kernel, jpeg_huff_sync_kernel, jpeg_huff_write_kernel, jpeg_huff_dc_kernel; ms7[6] is no time: subsequence
 * decodes of the synchronisation per subsequence (1 = a serial decoder's work). */
int  yn_jpeg_entropy_timing(yn_handle* h, yn_jpeg* j, float* ms7);

/* ---- baseline JPEG encode: every stage on the device, the finished files come down ------------------------------------------------------
 * The files cv2.imwrite(path_jpg, frame) / PIL's save write with libjpeg's defaults (JDCT_ISLOW, the Annex K tables, no optimisation, JFIF
 * 1.01 header), byte for byte: three components, sampling 4:2:0 (jpeg_set_defaults), 4:2:2 or 4:4:4, numbered 2, 1, 0 as PIL numbers them. */
typedef struct yn_jpeg_enc yn_jpeg_enc;
/* Host only.  jpeg_set_quality(quality, TRUE): the luma and chroma tables for quality 1..100, [2][64] in natural order.  1 = bad argument. */
int  yn_jpeg_quant_tables(int quality, uint16_t* qt2x64_natural);
/* Host only, no handle, no GPU.  The 623 bytes libjpeg writes before the entropy-coded data: SOI, JFIF APP0, two DQT, SOF0, four DHT
 * (DC0, AC0, DC1, AC1), SOS.  1 = bad argument (a side outside 1..16384, quality outside 1..100, unknown sampling). */
int  yn_jpeg_header(int w, int h, int quality, int sampling, uint8_t* out623);
/* An encoder for the handle's device, for up to max_batch (1..1024) frames a call.  stream_bytes (1024..2^32) is the size of the output
 * buffer that receives the files of one call, and of the unstuffed bit stream beside it; the per-block buffers grow with the frames. */
int  yn_jpeg_enc_create(yn_handle* h, int max_batch, int64_t stream_bytes, yn_jpeg_enc** out);
void yn_jpeg_enc_destroy(yn_jpeg_enc* enc);
/* cv2.imwrite's compression for n frames at once: frames_host[i] is a DEVICE pointer to uint8 [h_i][w_i][3] BGR, geom_host [n][2] = w_i, h_i.
 * Returns once the work is enqueued on the handle's stream.  Refused (1) before anything is launched, naming the image where there is one:
 * null pointers, n above max_batch, a side outside 1..16384, a quality outside 1..100, an unknown sampling, a batch of more than 2^24 blocks
 * (the worst case of its unstuffed stream cannot be staged).  A refused call leaves the previous batch as it was: it can still be
 * fetched.  n == 0 is no error: it leaves an empty batch. */
int  yn_jpeg_encode_batch(yn_handle* h, yn_jpeg_enc* enc, int n, const uint8_t* const* frames_host, const int32_t* geom_host, int quality, int sampling);
/* Synchronises.  offsets_host [n + 1]: file i of the last batch is files_host[offsets[i] .. offsets[i + 1]); one read-back of the offsets, one
 * copy of offsets[n] bytes.  An image whose file did not fit the encoder's buffers was not written at all: the call fails (1), naming the
 * image and the bytes the batch needs; so it does when cap is below offsets[n] (offsets_host is filled either way). */
int  yn_jpeg_encode_fetch(yn_handle* h, yn_jpeg_enc* enc, int64_t* offsets_host, uint8_t* files_host, int64_t cap);
/* Testing aid (synchronises): the quantised coefficients of image i of the last batch, in exactly yn_jpeg_coefficients' layout. */
int  yn_jpeg_enc_coefficients(yn_handle* h, yn_jpeg_enc* enc, int i, int16_t* host, int64_t cap);
/* Testing aid (synchronises): the 64 bytes the encoder keeps behind its output buffer; every one is 0xA5 unless something wrote out of bounds. */
int  yn_jpeg_enc_guard(yn_handle* h, yn_jpeg_enc* enc, uint8_t* host64);
/* Measurement (synchronises): ms10 = HIP event times of the last batch: table upload + clearing the stream, fdct, bits, scan tiles, scan sums
 * + stream layout, emit, 0xFF count, scan tiles, scan sums + file layout, files. */
int  yn_jpeg_enc_timing(yn_handle* h, yn_jpeg_enc* enc, float* ms10);

/* ---- measurement -------------------------------------------------------------------------- */
/* When enabled, every kernel launch of yn_forward_raw / yn_infer is bracketed by a pair of HIP
 * events recorded on the handle's stream (graph replay is bypassed while enabled).  After the
 * call, yn_profile_get(i) returns the launch's layer name, the kernel symbol, its measured duration and its
 * ALGORITHMIC flops / bytes (each conv reads its input once and writes its output once, weights
 * once — DESIGN.md §Measurement).  bench.py builds its `roofline` block from these. */
int  yn_profile_enable(yn_handle* h, int enable);
int  yn_profile_count(yn_handle* h);
int  yn_profile_get(yn_handle* h, int i, char* name, int name_cap, char* kernel, int kernel_cap,
                    float* ms, double* alg_flops, double* alg_bytes);

#ifdef __cplusplus
}
#endif
#endif /* YOLONANO_HIP_H */
