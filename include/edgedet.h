/*
 * edgedet.h — C-ABI of libedgedet.so, the MI355X (gfx950) detection-output engine.
 *
 * This library is the native half of the drop-in replacement for the hot path of
 * torch_models/detect.py (the torchvision forward called at detect.py:78 for the models built by
 * load_weak_models, detect.py:15-42).  The reference has no FFI of its own (no native
 * code); its operator boundary is the torchvision detection-model call
 *     model(Tensor[N,3,H,W] float32 in [0,1]) -> List[{"boxes","scores","labels"}]   (detect.py:78-81)
 * and the torchvision C++ operators that call reaches (torchvision::nms, torchvision::roi_align and the
 * ATen convolutions).  Each entry point below names the reference operator it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with `host_`;
 *   - the caller owns every buffer (images, packed weights, workspace, outputs); nothing here
 *     allocates on the hot path;
 *   - every call is asynchronous on the given stream (hipStream_t passed as void*; NULL = default);
 *   - return value: 0 = ok, < 0 = error; edgedet_last_error() returns the message (thread-local).
 *   - activations are NHWC float32; boxes are (x1, y1, x2, y2) float32.
 */
#ifndef EDGEDET_H
#define EDGEDET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------- plan ops */
/*
 * One step of a static execution plan.  The Python host (edgeml_amd/plan.py) lowers a detector
 * into an array of these (BatchNorm folded, weights packed, buffers carved from one arena) and the
 * native executor launches them in order.  Field meaning per `kind` is documented in
 * csrc/records.hpp; sizes and pointers are plain integers so the layout is identical from ctypes.
 */
#define EDGEDET_OP_INTS 48
#define EDGEDET_OP_PTRS 24
#define EDGEDET_OP_DBLS 8
#define EDGEDET_OP_FLTS 16

/* One op record.  Field layouts per kind: csrc/records.hpp (the named slots), e.g. DWCONV p0 x, p1 w,
 * p2 bias, p3 y, p4 SE partial sums; GROUP i0 = members. */
typedef struct edgedet_op {
    int64_t kind;
    int64_t i[EDGEDET_OP_INTS];
    uint64_t p[EDGEDET_OP_PTRS];
    double d[EDGEDET_OP_DBLS]; /* thresholds compared in double, as the reference's CPU nms */
    float f[EDGEDET_OP_FLTS];
} edgedet_op;

enum {
    EDGEDET_OP_MEMSET = 1,        /* zero p[0] for i[0] bytes                                         */
    EDGEDET_OP_PREPROCESS = 2,    /* GeneralizedRCNNTransform: normalize, bilinear resize, zero pad   */
    EDGEDET_OP_CONV = 3,          /* conv2d + folded BN + bias + residual/upsample-add + activation   */
    EDGEDET_OP_DWCONV = 4,        /* depthwise conv2d + folded BN + activation (+ the SE squeeze)      */
    EDGEDET_OP_CHANNEL_MEAN = 5,  /* adaptive_avg_pool2d(1) (SqueezeExcitation squeeze)               */
    EDGEDET_OP_SE_FC = 6,         /* SqueezeExcitation fc1-ReLU-fc2-Hardsigmoid (standalone form)      */
    EDGEDET_OP_MAXPOOL = 7,       /* max_pool2d (ResNet stem 3x3 s2 p1, FPN LastLevelMaxPool 1x1 s2)  */
    EDGEDET_OP_SSD_SCORES = 8,    /* SSD softmax + BoxCoder.decode + clip                             */
    EDGEDET_OP_SSD_CLASS_NMS = 9, /* per (image, class): score>t, top-k, NMS                          */
    EDGEDET_OP_MERGE_TOPK = 10,   /* per image: merge kept lists, sort by score, keep[:N], rescale    */
    EDGEDET_OP_RPN_LEVEL_NMS = 11,/* per (image, FPN level): top-k logits, decode, clip, small, NMS
                                   * (with p20..p22 a chunked top-k: per-chunk lists first; with p23
                                   * the NMS split into selection / IoU mask / scan launches)        */
    EDGEDET_OP_ROI_ALIGN = 12,    /* MultiScaleRoIAlign (LevelMapper + roi_align 7x7, sr=2)          */
    EDGEDET_OP_BOX_SCORES = 13,   /* RoIHeads softmax + class-specific decode + clip                 */
    EDGEDET_OP_BOX_CLASS_NMS = 14,/* per (image, class): score>t, remove_small, NMS                   */
    EDGEDET_OP_FORK = 15,         /* side lanes 1..i[0] wait for everything issued so far on lane 0    */
    EDGEDET_OP_JOIN = 16,         /* lane 0 waits for everything issued so far on lanes 1..i[0]        */
    EDGEDET_OP_SSD_POSTPROCESS = 17,/* per image: class top-k pool, global-order greedy NMS, [:N]      */
    EDGEDET_OP_GN_STATS = 18,     /* GroupNorm statistics -> per (image, channel) scale / shift       */
    EDGEDET_OP_RETINA_SELECT = 19,/* RetinaNet per (image, level): sigmoid > t, top-k, decode, clip   */
    EDGEDET_OP_RETINA_CLASS_NMS = 20,/* RetinaNet per (image, class): NMS over the level candidates  */
    EDGEDET_OP_SSD_STEM = 21,     /* SSDLite features.0.0 + features.0.1 in one pass                  */
    EDGEDET_OP_MBCONV = 22,       /* InvertedResidual without SE: expand, depthwise, project, residual */
    EDGEDET_OP_WAIT = 23,         /* lane i[0] waits for everything issued so far on lane i[1]         */
    /* 24 is retired (round 3's grouped SSD head kernel, measured slower and removed) */
    EDGEDET_OP_GROUP = 25         /* the next i[0] records (all CONV or all DWCONV, same lane) issued as ONE
                                   * grouped kernel launch; each member stays a complete record (and is
                                   * issued alone when the members cannot share a kernel variant) */
};

/* i[EDGEDET_OP_LANE] of every record selects the stream it is issued on: 0 = the caller's stream,
 * 1..3 = side streams owned by the library (joined back by EDGEDET_OP_JOIN; captured graphs keep
 * the fork/join as graph dependencies). */
#define EDGEDET_OP_LANE 47
#define EDGEDET_MAX_LANES 4
/* members of one EDGEDET_OP_GROUP launch */
#define EDGEDET_MAX_GROUP 12

/* Run ops[0..n) on `stream`.  Shapes are checked on the host before any launch; the lane topology
 * (FORK / JOIN / WAIT and every record's lane) is checked before anything is issued. */
int edgedet_plan_run(const edgedet_op* ops, int64_t n, void* stream);
/* The lane-topology check alone (no device access): 0 or the error edgedet_plan_run would return. */
int edgedet_plan_check(const edgedet_op* ops, int64_t n);
/* The library keeps side lanes (3 streams + events) per caller stream, at most 16 sets per device: a
 * new caller stream beyond that takes over the least recently used set (sets are never destroyed:
 * captured graphs refer to them).  edgedet_release_lanes marks `stream`'s set as the next to be taken
 * over; edgedet_lane_sets returns the number of sets. */
int edgedet_release_lanes(void* stream);
int64_t edgedet_lane_sets(void);

/* Capture ops[0..n) into a hipGraph (instantiated); *graph receives an opaque handle. */
int edgedet_graph_create(const edgedet_op* ops, int64_t n, void* stream, void** graph);
int edgedet_graph_launch(void* graph, void* stream);
int edgedet_graph_destroy(void* graph);

/* Diagnostic: leave `bytes` (a multiple of 256, 0 = none, the default) unused before, between and after
 * the workspace buffers of every plan looked up from now on (the redzone is part of the plan cache key,
 * so layouts with and without gaps never mix), so a caller can fill the gaps with a canary and catch a
 * kernel writing outside its buffers (tests/test_gpu_redzone.py).  The layout changes with the
 * setting: query edgedet_model_workspace_size and run edgedet_model_prepare again after every call
 * before the next forward -- a workspace sized before the switch is too small for the new layout. */
int edgedet_set_redzone(int64_t bytes);

/* ------------------------------------------------------------------------ model forward */
/*
 * The detector call of torch_models/detect.py:78 (model(images) -> boxes / scores / labels for the
 * models load_weak_models builds, detect.py:15-42), natively: the library lowers the detector into
 * the same static plan the Python host builds (edgeml_amd/models.py; results bit-identical to it).
 *   kind         EDGEDET_MODEL_SSDLITE (ssdlite320_mobilenet_v3_large, detect.py:24/26; reduced_tail
 *                1 = the COCO-pretrained variant, 0 = the --model-path / train.py variant) or
 *                EDGEDET_MODEL_FRCNN (fasterrcnn_resnet50_fpn_v2, detect.py:30/32; reduced_tail unused) or
 *                EDGEDET_MODEL_RETINANET (retinanet_resnet50_fpn_v2, detect.py:36/38, the CLI's third model)
 *   num_classes  91 (coco) or 21 (voc), detect.py:67
 * Weights: edgedet_model_pack packs torchvision-named host tensors (a state_dict: names, fp32 values,
 * element counts; num_batches_tracked may be omitted) into a blob of edgedet_model_weights_size bytes
 * (BatchNorm folded, conv weights repacked and split into bf16 planes), which the caller copies to
 * the device once.  Images: B x [3, H, W], float in [0, 1] (input_u8 = 0, detect.py:58) or the
 * decoded uint8 bytes (input_u8 = 1, divided by 255 on the device, bit-identical).  Workspace:
 * caller-owned device memory of edgedet_model_workspace_size bytes for (B, H, W, input_u8), set up
 * once by edgedet_model_prepare (zeroes it and writes the anchors / rescale constants; synchronous).  Outputs:
 * count [B] int32, boxes [B][K][4] xyxy float in original pixels, scores [B][K] descending,
 * labels [B][K] int64, K = edgedet_model_max_detections(kind) (300 SSD / 100 FRCNN / 300 RetinaNet), the first
 * count[b] rows valid (detect.py:79-81).  forward is asynchronous on `stream`.
 */
enum { EDGEDET_MODEL_SSDLITE = 0, EDGEDET_MODEL_FRCNN = 1, EDGEDET_MODEL_RETINANET = 2 };
int64_t edgedet_model_weights_size(int32_t kind, int32_t num_classes, int32_t reduced_tail);
int edgedet_model_pack(int32_t kind, int32_t num_classes, int32_t reduced_tail, int64_t n_params,
                       const char* const* names, const float* const* host_values, const int64_t* numels,
                       void* host_blob);
int64_t edgedet_model_workspace_size(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B,
                                     int32_t H, int32_t W, int32_t input_u8);
int edgedet_model_prepare(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                          int32_t W, int32_t input_u8, void* workspace, void* stream);
/* edgedet_model_prepare into a host image of the workspace (bytes >= the workspace size): the
 * constants at their offsets, nothing else written (host-side checks and staging). */
int edgedet_model_prepare_host(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                               int32_t W, int32_t input_u8, void* host_workspace, int64_t bytes);
int edgedet_model_forward(int32_t kind, int32_t num_classes, int32_t reduced_tail, const void* weights,
                          const void* images, int32_t B, int32_t H, int32_t W, int32_t input_u8,
                          void* workspace, int32_t* count, float* boxes, float* scores, int64_t* labels,
                          void* stream);
int edgedet_model_max_detections(int32_t kind);
/* The workspace buffers of the plan (name, byte offset into the workspace, element type, shape): what a
 * host reads back for inspection (the parity tests read the head outputs, scores, proposals ...).
 * Returns the buffer count; fills out[] when cap is large enough. */
enum { EDGEDET_DT_F32 = 0, EDGEDET_DT_I32 = 1, EDGEDET_DT_I64 = 2, EDGEDET_DT_U8 = 3, EDGEDET_DT_I16 = 4 };
typedef struct edgedet_buffer {
    char name[96];
    int64_t offset;  /* bytes from the workspace base */
    int64_t nbytes;
    int32_t dtype;   /* EDGEDET_DT_* */
    int32_t ndim;
    int64_t shape[6];
} edgedet_buffer;
int64_t edgedet_model_buffers(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                              int32_t W, int32_t input_u8, edgedet_buffer* out, int64_t cap);
/* The layer name of every record ('\n'-separated, torchvision module paths): returns the bytes needed
 * (including the terminating NUL); fills out when cap is large enough. */
int64_t edgedet_model_op_names(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                               int32_t W, int32_t input_u8, char* out, int64_t cap);
/* Drop the cached plan of (B, H, W, input dtype) (at most 64 plans per model are kept, least recently
 * used evicted; records and workspaces already handed out stay valid). */
int edgedet_model_release(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H, int32_t W,
                          int32_t input_u8);
/* The op records forward would run (for graph capture: edgedet_graph_create on them, and for tests);
 * pointers resolved against the given bases (0 = the workspace's own region for images / outputs).
 * Returns the record count; fills out[] when cap is large enough. */
int64_t edgedet_model_records(int32_t kind, int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                              int32_t W, int32_t input_u8, uint64_t weights, uint64_t workspace,
                              uint64_t images, uint64_t count, uint64_t boxes, uint64_t scores,
                              uint64_t labels, edgedet_op* out, int64_t cap);
/* The per-detector names: the calls above with kind fixed. */
int64_t edgedet_ssdlite_workspace_size(int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H,
                                       int32_t W, int32_t input_u8);
int edgedet_ssdlite_forward(const void* weights, int32_t num_classes, int32_t reduced_tail, const void* images,
                            int32_t B, int32_t H, int32_t W, int32_t input_u8, void* workspace,
                            int32_t* count, float* boxes, float* scores, int64_t* labels, void* stream);
int64_t edgedet_frcnn_workspace_size(int32_t num_classes, int32_t B, int32_t H, int32_t W, int32_t input_u8);
int edgedet_frcnn_forward(const void* weights, int32_t num_classes, const void* images, int32_t B, int32_t H,
                          int32_t W, int32_t input_u8, void* workspace, int32_t* count, float* boxes,
                          float* scores, int64_t* labels, void* stream);

/* ------------------------------------------------------------------------ unit operators */
/*
 * torchvision::nms (reference call sites: SSD postprocess, RPN filter_proposals and RoIHeads
 * postprocess_detections, all reached from detect.py:78; semantics SURVEY.md App. A.0).
 * boxes [n,4], scores [n] -> keep [n] int64 (indices, score-descending, ties lower index first),
 * *d_num_keep int32.  Suppress j when inter/(area_i+area_j-inter) > iou_threshold.  n <= 524288:
 * up to 1024 boxes one workgroup does it all; above, a radix sort, a tiled IoU bitmask and a blocked
 * greedy scan (csrc/unitops.hip).  The scratch grows QUADRATICALLY with n: the IoU bitmask alone is
 * 8 * n * ceil(n / 64) bytes (0.5 GB at n = 65,536; 34 GB at the 524,288 cap, which fits MI355X's
 * 288 GB), plus about 40 bytes per box.  edgedet_nms / edgedet_batched_nms are CONVENIENCE entry
 * points: they take that scratch from the stream-ordered allocator (hipMallocAsync on `stream`), so
 * they allocate on the calling path.  The hot path (the model plans) never calls them; a caller that
 * must not allocate uses the _ws variants with caller-owned scratch of edgedet_nms_workspace_size(n)
 * bytes instead.
 */
int edgedet_nms(const float* boxes, const float* scores, int64_t n, double iou_threshold,
                int64_t* keep, int32_t* d_num_keep, void* stream);

/*
 * torchvision::ops.batched_nms (per-group greedy NMS; result sorted by score descending, ties by
 * lower index).  Equivalent to the reference's _batched_nms_vanilla.  n <= 524288 (as edgedet_nms).
 */
int edgedet_batched_nms(const float* boxes, const float* scores, const int64_t* idxs, int64_t n,
                        double iou_threshold, int64_t* keep, int32_t* d_num_keep, void* stream);
int64_t edgedet_nms_workspace_size(int64_t n);
int edgedet_nms_ws(const float* boxes, const float* scores, int64_t n, double iou_threshold, int64_t* keep,
                   int32_t* d_num_keep, void* workspace, int64_t workspace_bytes, void* stream);
int edgedet_batched_nms_ws(const float* boxes, const float* scores, const int64_t* idxs, int64_t n,
                           double iou_threshold, int64_t* keep, int32_t* d_num_keep, void* workspace,
                           int64_t workspace_bytes, void* stream);

/*
 * torch.topk per segment (RPN filter_proposals' per-level pre_nms_top_n, SSD's per-class topk of
 * postprocess_detections; reached from detect.py:78): segment s is values[seg_off[s] .. seg_off[s+1]);
 * out_values / out_index [nseg][k] (index within the segment), out_count[s] = min(k, length).  Values
 * descending, ties lower index first (the rule the oracle fixes).  1 <= k <= 1024.
 */
int edgedet_topk_segments(const float* values, const int64_t* seg_off, int64_t nseg, int32_t k,
                          float* out_values, int64_t* out_index, int32_t* out_count, void* stream);

/*
 * torchvision BoxCoder.decode_single: deltas [n,4] against ref_boxes [n,4] (xyxy)
 * with weights (wx, wy, ww, wh), dw / dh clamped to <= clamp (log(1000/16) in torchvision); then
 * clip_boxes_to_image to [0, img_w] x [0, img_h] when both are > 0.  out [n,4]; 16-byte aligned rows.
 */
int edgedet_box_decode(const float* deltas, const float* ref_boxes, int64_t n, float wx, float wy, float ww,
                       float wh, float clamp, float img_h, float img_w, float* out, void* stream);

/*
 * torchvision::roi_align forward, aligned=False (MultiScaleRoIAlign's call),
 * on an NHWC feature map.  feat [B,H,W,C]; rois [R,5] (batch_idx, x1, y1, x2, y2);
 * out [R,PH,PW,C] (NHWC; the reference's NCHW output permuted).
 */
int edgedet_roi_align(const float* feat, int64_t B, int64_t H, int64_t W, int64_t C,
                      const float* rois, int64_t R, float spatial_scale, int32_t pooled_h,
                      int32_t pooled_w, int32_t sampling_ratio, float* out, void* stream);

/*
 * ATen conv2d (+ eval BatchNorm folded into w/bias, + activation), the layers of the torchvision
 * backbones/heads reached from detect.py:78.  x NHWC [B,H,W,Cin]; w [Cout][KH][KW][Cin] (packed:
 * K = KH*KW*Cin padded to a multiple of 32 with zeros, see edgedet_conv_weight_k); bias [Cout];
 * res (nullable) NHWC [B,Ho,Wo,Cout] added before the activation; y NHWC [B,Ho,Wo,Cout].
 * act: 0 none, 1 relu, 2 relu6, 3 hardswish, 4 hardsigmoid, 5 sigmoid.
 */
int edgedet_conv2d(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                   const float* bias, int64_t Cout, int32_t KH, int32_t KW, int32_t stride,
                   int32_t pad, int32_t act, const float* res, float* y, void* stream);
int64_t edgedet_conv_weight_k(int32_t KH, int32_t KW, int64_t Cin);

/*
 * edgedet_conv2d with the math selectable: w3 (nullable) holds the packed weight split into three
 * bf16 planes [3][Cout][Kpad] (edgedet_split_bf16x3).  With w3 the compute-bound tiles run the
 * fp32 GEMM on the bf16 matrix cores as six partial products (error below one fp32 rounding per
 * product, csrc/conv.hip "bf16x6"); without it they run v_mfma_f32_32x32x2_f32.  tile 0 = auto.
 */
int edgedet_conv2d_ex(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                      const uint16_t* w3, const float* bias, int64_t Cout, int32_t KH, int32_t KW,
                      int32_t stride, int32_t pad, int32_t act, const float* res, float* y, int32_t tile,
                      void* stream);
/*
 * edgedet_conv2d_ex with a caller-owned scratch x3 of 3 * B*H*W*Cin + 32 uint16: when the 256 x 128
 * bf16x6 tile runs (tile 25, Cin % 32 == 0) the input is split into three bf16 planes once, by a
 * separate pass into x3, instead of inside every N tile of the GEMM.  Results are bit-identical to
 * edgedet_conv2d_ex; x3 may be null (then this is edgedet_conv2d_ex).
 */
int edgedet_conv2d_x3(const float* x, uint16_t* x3, int64_t B, int64_t H, int64_t W, int64_t Cin,
                      const float* w, const uint16_t* w3, const float* bias, int64_t Cout, int32_t KH,
                      int32_t KW, int32_t stride, int32_t pad, int32_t act, const float* res, float* y,
                      int32_t tile, void* stream);
/* Packed weights w [n / kpad][kpad] fp32 -> out [3][n] bf16 bit patterns: x0 = RN(x), x1 = RN(x - x0),
 * x2 = x - x0 - x1 (exact), of x = w, and of x = -w in the odd 32-wide K blocks (k / 32 odd): the
 * bf16x6 kernels subtract those stages' sums, which cancels the matrix cores' truncation bias
 * (csrc/conv.hip conv_x6b_body).  kpad: a multiple of 32 dividing n. */
int edgedet_split_bf16x3(const float* w, int64_t n, int64_t kpad, uint16_t* out, void* stream);

/*
 * SSDLite stem + first block in one pass: y = proj(relu(dw3x3(s))) + b1 + s with
 * s = hardswish(conv3x3_s2(x) + b0) (torchvision mobilenet_v3_large features.0.0 and .0.1, folded BN).
 * x NHWC4 [B,H,W,4] (the preprocessed image); w0 [16][ld0] packed (kh, kw, ci); wd [9][16];
 * w1 [16][ld1]; y [B,(H+1)/2,(W+1)/2,16].
 */
int edgedet_ssd_stem(const float* x, int64_t B, int64_t H, int64_t W, const float* w0, int64_t ld0,
                     const float* b0, const float* wd, const float* bd, const float* w1, int64_t ld1,
                     const float* b1, float* y, void* stream);
/*
 * ORIE estimator (regression.py:242-355 fit_CNN on the stage-24 features, lib/nn_model.py:28-112
 * with linear stacks only): an MLP dims[0] -> ... -> dims[L] = 1 whose hidden layers are Linear,
 * BatchNorm1d, ReLU, Dropout(dropout); MSE loss (reward-weighted when `weighted`), Adam(lr,
 * weight_decay), MultiStepLR(milestones, gamma), `batch` rows in index order, a test pass on the
 * validation rows after every epoch.  One workgroup per fold f trains on rows tr_idx[tr_off[f] ..
 * tr_off[f+1]) with targets y[f][.] and tests on va_idx[va_off[f] .. va_off[f+1]).  State vectors
 * ([F][edgedet_mlp_state_size]: per layer W, b, and for hidden layers gamma, beta; then the running
 * mean / var) start from init; best (lowest test loss) and last are written; adam is [F][2 * params]
 * scratch; train_loss / test_loss are [F][epochs].  dims and milestones are host arrays.
 */
int64_t edgedet_mlp_state_size(int32_t L, const int32_t* dims);
int edgedet_mlp_fit(const float* x, int64_t N, int64_t D0, const float* y, const int32_t* tr_idx,
                    const int64_t* tr_off, const int32_t* va_idx, const int64_t* va_off, int32_t folds, int32_t L,
                    const int32_t* dims, const float* init, float* best, float* last, float* adam,
                    float* train_loss, float* test_loss, int32_t epochs, int32_t batch, float lr, float gamma,
                    const int32_t* milestones, int32_t n_milestones, float weight_decay, int32_t weighted,
                    float dropout, uint64_t seed, void* stream);
/* Eval-mode forward of a trained state (running statistics, no dropout): out[r] = net(x[idx[r]]). */
int edgedet_mlp_predict(const float* x, int64_t D0, const int32_t* idx, int64_t n, int32_t L, const int32_t* dims,
                        const float* state, float* out, void* stream);
/* Depthwise conv2d (+ folded BN + act).  x NHWC [B,H,W,C]; w [KH*KW][C]; bias [C]. */
int edgedet_dwconv2d(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* w,
                     const float* bias, int32_t K, int32_t stride, int32_t pad, int32_t act,
                     float* y, void* stream);

/* The conv kernel variant (tile id of csrc/conv.hip conv_launch: 1-6 fp32-MFMA LDS tiles, 10-12 and
 * 15 direct pointwise tiles, 13/14/16/17 split-K pointwise tiles, 21-24/27/28 bf16x6 16-deep LDS tiles,
 * 25/26, 29-32, 38 and 39 bf16x6 32-deep swizzled tiles: 256x128 (26 with split K), 128x128, 64x128,
 * 128x64, 128x256, 33-35 streaming 1x1 tiles for Cin <= 72, Cout <= 96 with dense output rows) that a CONV
 * record would run; negative on error. */
int edgedet_conv_tile(const edgedet_op* op);

/* ------------------------------------------------------------------ ORIE consumer (reward.py) */
/*
 * lib/metrics.py box_correct (lib/data.py set_data's TP flags) for many images at once: detections
 * det_xyxy [n_det][4] f64 + det_cls, labels lab_xyxy [n_lab][4] f64 + lab_cls, both grouped per image
 * by the offsets det_off / lab_off [n_img + 1]; tp [n_det] = 1 where the detection is matched at
 * IoU >= iou_thr.  max_labels = the most labels of any one image (any count; images with more than
 * 1024 labels are matched in 1024-label chunks).
 */
int edgedet_box_correct(const double* det_xyxy, const int32_t* det_cls, const int64_t* det_off,
                        const double* lab_xyxy, const int32_t* lab_cls, const int64_t* lab_off,
                        int64_t n_img, double iou_thr, uint8_t* tp, int64_t max_labels, void* stream);
/*
 * reward.py compute_orie's two ap_per_class calls (lib/metrics.py:89-148) for n_eval evaluations.
 * Entries = every detection of every image (weak and strong), sorted per class by (conf desc, image,
 * row, weak before strong); ent_img [n_ent], ent_flag [n_ent] (bit0 TP, bit1 strong), class segments
 * seg_off [n_cls + 1]; lab_cnt [n_img][n_cls] labels per image and class; evaluation e targets image
 * target[e] with ensemble ens[e][0..E) (target excluded).  ap [n_eval][2][n_cls] (weak, strong AP per
 * class, float64, bit-identical to numpy's), n_l [n_eval][n_cls] (labels of the class in the ensemble
 * plus the target; the reference's unique classes are those with n_l > 0).
 */
int edgedet_orie_ap(const int32_t* ent_img, const uint8_t* ent_flag, const int64_t* seg_off, int32_t n_cls,
                    const int32_t* lab_cnt, int64_t n_img, const int32_t* target, const int32_t* ens, int32_t E,
                    int64_t n_eval, double* ap, int32_t* n_l, void* stream);
/*
 * test.py test_map's ap_per_class over a weak/strong mixture (test.py:14-44): evaluation e uses the
 * weak detections of the images set in weak_mask[e] and the strong detections of those in
 * strong_mask[e] (bitmaps [n_eval][(n_img + 31) / 32], bit i of word i / 32).  Same entries, AP
 * layout (ap[e][0][c]) and n_l as edgedet_orie_ap.
 */
int edgedet_map_eval(const int32_t* ent_img, const uint8_t* ent_flag, const int64_t* seg_off, int32_t n_cls,
                     const int32_t* lab_cnt, int64_t n_img, const uint32_t* weak_mask, const uint32_t* strong_mask,
                     int64_t n_eval, double* ap, int32_t* n_l, void* stream);

/*
 * lib/data.py:127-160 extract_output_feature for n_img images at once: rows [n][ncol] f64 (each
 * image's detection-file rows, grouped by off [n_img + 1]); out [n_img][num_class + (ncol - 1) * k]:
 * class counts of the first k rows, then their columns 1.. flattened (zeros beyond).
 */
int edgedet_output_features(const double* rows, const int64_t* off, int64_t n_img, int32_t ncol, int32_t num_class,
                            int32_t k, double* out, void* stream);

/* ------------------------------------------------------------------ comparison baselines (baseline.py) */
/*
 * baseline.py:67-152 fit_dcsb for every cross-validation fold in one launch (a workgroup per fold),
 * bit-exact: float64 and integer arithmetic only.  conf / area [n_det] are every image's detections
 * (grouped by det_off [N + 1]); fold f trains on images tr_idx[tr_off[f] .. tr_off[f+1]); label_num [N]
 * labels per image; reward [N] 0 / 1; grid [n_grid <= 128] the area thresholds (np.arange(0.2, 0.9, 0.01),
 * computed by the caller).  Scratch: ws_num [F][2][N] int32, ws_area [F][N].  Writes per fold
 * thresh = (conf_thresh, area_thresh), num_thresh, est [F][N] (the estimate of every image, training and
 * validation), steps (bisection halvings) and status: 0 ok, 1 the confidence bisection did not meet
 * the reference's stopping rule within 64 halvings (the reference loops forever there), 2 no grid
 * cell has a positive accuracy.
 */
int edgedet_dcsb_fit(const double* conf, const double* area, const int64_t* det_off, int64_t N,
                     const int64_t* label_num, const int32_t* reward, const int32_t* tr_idx, const int64_t* tr_off,
                     int32_t folds, const double* grid, int32_t n_grid, int32_t* ws_num, double* ws_area,
                     double* thresh, int32_t* num_thresh, int32_t* est, int32_t* status, int32_t* steps,
                     void* stream);
/*
 * baseline.py:29-64 fit_af: the optimum of LinearSVC(dual=False, class_weight={0: 1, 1: pos_weight}),
 * f(v) = 1/2 |v|^2 + sum_i C_i max(0, 1 - s_i v.x_i)^2, per fold by a damped Newton method in float64
 * (Hessian by the fp64 matrix instruction, Cholesky, Armijo line search).  x [N][Dp]: the features, a
 * column of ones (the regularised bias) and zero columns up to Dp, a multiple of 16, <= 256; y [N]
 * 0 / 1; tr_off_host is the host copy of the device array tr_off [F + 1].  v [F][Dp] holds the start
 * (zeros) and receives the solution; ws: edgedet_svm_workspace_size bytes, total_rows = tr_off[F].
 * Stops a fold at |grad f| <= tol or after max_iter Newton steps; writes iters, gnorm (the last
 * gradient norm) and status (0 ok, 1 not converged, 2 line search failed, 3 Hessian not positive
 * definite) per fold.  Synchronises the stream: the iteration count is decided on the device.
 */
int64_t edgedet_svm_workspace_size(int32_t folds, int64_t Dp, int64_t total_rows);
int edgedet_svm_fit(const double* x, int64_t N, int64_t Dp, const int32_t* y, double pos_weight,
                    const int32_t* tr_idx, const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, double* v,
                    void* ws, int64_t ws_bytes, int32_t max_iter, double tol, int32_t* iters, double* gnorm,
                    int32_t* status, void* stream);
/* The solver's Hessian as a unit operator: H [Dp][Dp] = I + sum_r w[r] x[idx[r]] x[idx[r]]^T over n rows
 * (idx null: rows 0..n), both triangles written. */
int edgedet_svm_hessian(const double* x, int64_t Dp, const int32_t* idx, int64_t n, const double* w, double* H,
                        void* stream);
/* out [F][N] = x v[f]: the decision value of every row under every fold's model. */
int edgedet_svm_decision(const double* x, int64_t N, int64_t Dp, const double* v, int32_t folds, double* out,
                         void* stream);

/* ------------------------------------------------------------------ estimator regressors (regression.py) */
/*
 * regression.py's LinearRegression, ElasticNet, BayesianRidge and KNeighborsRegressor behind fit_model's
 * StandardScaler (:38-77), float64, every cross-validation fold in flight (csrc/regress.hip).  Common
 * arguments: x [N][D] the raw features (1 <= D <= 255), y [F][N] the target of every row under every fold,
 * fold f trains on rows tr_idx[tr_off[f] .. tr_off[f+1]) (tr_idx null: on rows tr_off[f] .. tr_off[f+1]
 * themselves); tr_off_host is the host copy of the device array tr_off [F + 1].  Dp = D + 1 rounded up to
 * a multiple of 16.  Every function checks its shapes on the host and returns 0 or a negative error code
 * (edgedet_last_error); iterative solvers report a status per fold.
 *
 * edgedet_reg_workspace_size: bytes of the workspace of edgedet_reg_eigh (N = total_rows = 0) or of
 * edgedet_knn_fit_predict (total_rows = tr_off[F]); < 0 on bad sizes.
 */
int64_t edgedet_reg_workspace_size(int32_t folds, int64_t D, int64_t N, int64_t total_rows);
/* StandardScaler.fit per fold: mean [F][D], scale [F][D] = sqrt(population variance), 1 for a column that
 * sklearn's _is_constant_feature calls constant (var <= n eps var + (n mean eps)^2); ymean [F] the mean of
 * the fold's training targets (0 when y is null). */
int edgedet_reg_scaler(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                       const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, double* mean, double* scale,
                       double* ymean, void* stream);
/* G [F][Dp][Dp] = Z~^T Z~ over the fold's training rows by the fp64 matrix instruction, both triangles
 * written: Z~ = ((x - mean) * (1 / scale), y - ymean, 0 ...), so G[:D,:D] = Z^T Z, G[:D,D] = Z^T yc and
 * G[D,D] = yc^T yc (y null: that column is zero).  With folds = 1 and tr_idx null it is the unit operator
 * for one matrix. */
int edgedet_reg_gram(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                     const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                     const double* scale, const double* ymean, double* G, void* stream);
/* Symmetric eigendecomposition of G[f][:D,:D] (cyclic parallel Jacobi, one workgroup per fold): lam [F][D]
 * the eigenvalues clamped at 0 in the solver's order, vt [F][D][D] with row i the eigenvector of lam[i].
 * Iterates until the off-diagonal norm is <= D eps |G|_F; offnorm [F][2] = {the final off-diagonal norm,
 * that threshold}, sweeps [F], status [F]: 0 ok, 1 not converged in max_sweeps. */
int edgedet_reg_eigh(const double* G, int64_t D, int32_t folds, void* ws, int64_t ws_bytes, int32_t max_sweeps,
                     double* lam, double* vt, int32_t* sweeps, int32_t* status, double* offnorm, void* stream);
/* LinearRegression: coef [F][D] = V+ diag(1 / lam+) V+^T Z^T yc over the eigenvalues lam > tau max(lam), the
 * minimum-norm least-squares solution; rank [F] their count, min_ratio [F] the smallest kept lam / max(lam). */
int edgedet_reg_fit_lr(const double* G, int64_t D, int32_t folds, const double* lam, const double* vt, double tau,
                       double* coef, int32_t* rank, double* min_ratio, void* stream);
/* BayesianRidge.fit (more training rows than features): sklearn's fixed-point loop in the eigenbasis, at
 * most max_iter iterations, stopped when sum |coef_old - coef| < tol (not tested on the first); coef [F][D],
 * hyper [F][2] = {alpha_, lambda_}, n_iter [F]. */
int edgedet_reg_fit_br(const double* G, int64_t D, const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds,
                       const double* lam, const double* vt, double alpha_1, double alpha_2, double lambda_1,
                       double lambda_2, double tol, int32_t max_iter, double* coef, double* hyper, int32_t* n_iter,
                       void* stream);
/* ElasticNet(alpha, l1_ratio < 1): covariance-form cyclic coordinate descent on Q = Z^T Z / n, stopped when
 * the optimality residual |z|_2 <= tol, tol = tol_abs when > 0, otherwise tol_rel |Z^T yc / n|_inf.
 * coef [F][D], res [F][2] = {|z|, tol}, sweeps [F], status [F]: 0 ok, 1 not converged in max_sweeps. */
int edgedet_reg_fit_en(const double* G, int64_t D, const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds,
                       double alpha, double l1_ratio, double tol_rel, double tol_abs, int32_t max_sweeps, double* coef,
                       double* res, int32_t* sweeps, int32_t* status, void* stream);
/* out [F][N] = ((x - mean) * (1 / scale)) . coef + ymean for every row under every fold's model. */
int edgedet_reg_predict(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                        const double* coef, const double* ymean, int32_t folds, double* out, void* stream);
/* KNeighborsRegressor(n_neighbors = k), brute force on the standardised rows: every row of the dataset is a
 * query against its fold's training rows.  Squared distances |a|^2 + |b|^2 - 2 a.b (clamped at 0) by the
 * fp64 matrix instruction, an exact k-smallest selection with ties at the k-th distance resolved to the
 * lowest training position; nbr [F][N][k] the neighbours' positions within the fold's training list in
 * ascending order, est [F][N] the mean of their targets summed in that order.  1 <= k <= every fold's
 * training rows. */
int edgedet_knn_fit_predict(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                            const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                            const double* scale, int32_t k, void* ws, int64_t ws_bytes, double* est, int32_t* nbr,
                            void* stream);

/* ------------------------------------------------------------------ support vector regressors (regression.py) */
/*
 * regression.py's SVR(kernel='rbf', C, epsilon) and LinearSVR(C, epsilon) behind fit_model's StandardScaler,
 * float64, every cross-validation fold in flight, each solved to the optimum of its strongly convex
 * objective (csrc/svr.hip).  x, y, tr_idx, tr_off_host, tr_off, folds, mean and scale are the
 * estimator regressors' (tr_idx is required; every fold non-empty; mean and scale from edgedet_reg_scaler).
 * With T = tr_off[F] the workspace holds Z [T][D], the standardised training rows of every fold, their
 * squared norms [T] and, for SVR, every fold's kernel matrix [n_f][n_f]; it is 8-byte aligned.
 *
 * edgedet_svr_workspace_size: its bytes (with_kernel != 0: for edgedet_svr_fit); < 0 on bad sizes.
 */
int64_t edgedet_svr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D, int32_t with_kernel);
/* The RBF kernel matrix of one matrix z [n][D], taken as it is: K [n][n] = exp(-gamma max(|a|^2 + |b|^2 -
 * 2 a.b, 0)) with the dot products by the fp64 matrix instruction; norm [n] receives |z_i|^2, gamma [1] the
 * value used: gamma_in when > 0, otherwise sklearn's gamma='scale', 1 / (D var), var the population variance
 * of all entries of z (1 when var is 0). */
int edgedet_svr_kernel_matrix(const double* z, int64_t n, int64_t D, double gamma_in, double* norm, double* gamma,
                              double* K, void* stream);
/* SVR: SMO on beta = alpha - alpha*, minimising 1/2 beta^T K beta - y^T beta + epsilon |beta|_1 on -C <= beta
 * <= C, sum beta = 0, with libsvm's second-order working-set selection, until libsvm's maximal KKT violation
 * m(beta) - M(beta) <= tol holds on a gradient recomputed from beta.  At most 4,000 training rows per fold.
 * beta [T] (fold f at tr_off[f]), intercept [F] (libsvm's rule), gamma [F] (gamma='scale'), viol [F] the final
 * violation, iters [F], status [F]: 0 ok, 1 not converged in max_iter.  The workspace keeps Z and the norms
 * for edgedet_svr_predict. */
int edgedet_svr_fit(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                    const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                    const double* scale, double C, double epsilon, double tol, int32_t max_iter, void* ws,
                    int64_t ws_bytes, double* beta, double* intercept, double* gamma, double* viol, int32_t* iters,
                    int32_t* status, void* stream);
/* out [F][N] = sum_j beta_j exp(-gamma_f |z - z_j|^2) + intercept_f for every row of x under every fold's
 * model, on the workspace edgedet_svr_fit filled: distance tiles, exponential and row sum in one kernel. */
int edgedet_svr_predict(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                        const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const void* ws,
                        int64_t ws_bytes, const double* beta, const double* intercept, const double* gamma,
                        double* out, void* stream);
/* LinearSVR (epsilon-insensitive loss, the bias a regularised feature of value 1): exact dual coordinate
 * descent in natural cyclic order, sixteen coordinates per block, until the duality gap P(X~^T beta) -
 * D(beta) <= tol, tol = tol_abs when > 0, otherwise tol_rel P(0).  beta [T], v [F][D + 1] = X~^T beta
 * recomputed from the final beta (coef = v[:D], intercept = v[D]: edgedet_reg_predict predicts), res [F][2] =
 * {gap, tol}, sweeps [F], status [F]: 0 ok, 1 not converged in max_sweeps. */
int edgedet_lsvr_fit(const double* x, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                     const int64_t* tr_off_host, const int64_t* tr_off, int32_t folds, const double* mean,
                     const double* scale, double C, double epsilon, double tol_abs, double tol_rel,
                     int32_t max_sweeps, void* ws, int64_t ws_bytes, double* beta, double* v, double* res,
                     int32_t* sweeps, int32_t* status, void* stream);

/* ------------------------------------------------------------------ prediction from saved SVR / KNR models */
/*
 * Estimates from the stored rows of a wts<k>.pickle (csrc/kpredict.hip, edgeml_amd.kpredict): an SVR file's
 * support vectors with their dual coefficients, or a KNR file's training rows with their targets.  Float64,
 * 1 <= D <= 255, fixed-order sums: the estimate of a feature row depends on the row and the model only, not on
 * B or on the row's place in feat.  Every function checks its arguments on the host and returns 0 or a
 * negative error code (edgedet_last_error) before anything is launched; the calls are asynchronous on `stream`.
 *
 * edgedet_kmodel_prepare, once per loaded model: z [n][D] = (rows - mean) * (1 / scale) and norm [n] = |z_i|^2
 * in the order edgedet_svr_fit and edgedet_knn_fit_predict use (sixteen lanes per row), so a KNR model
 * reproduces its fit bit for bit.  n = 0 is legal (an SVR without support vectors) and launches nothing.
 *
 * edgedet_kmodel_workspace_size: bytes of the workspace of a predict call on B rows (kind 0: SVR, one partial
 * sum per row and tile of sixteen support vectors; kind 1: KNR, the distances [B][n] and, for a call without
 * nbr, the selected positions); < 0 on bad sizes.  The workspace is 8-byte aligned.
 */
int edgedet_kmodel_prepare(const double* rows, int64_t n, int64_t D, const double* mean, const double* scale,
                           double* z, double* norm, void* stream);
int64_t edgedet_kmodel_workspace_size(int64_t n, int64_t D, int64_t B, int32_t kind);
/* est [B] = sum_j beta_j exp(-gamma max(|z_q|^2 + |z_j|^2 - 2 z_q.z_j, 0)) + intercept for the rows of feat
 * [B][D], standardised in the load: a wave per tile of 16 rows x 16 support vectors over the whole grid (dot
 * products by the fp64 matrix instruction), a tile's sixteen terms added by a butterfly, then a row's partial
 * sums added in an order that depends on n alone.  n = 0: est = intercept (z, norm and beta may be null). */
int edgedet_svr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean, const double* scale,
                              const double* z, const double* norm, const double* beta, int64_t n, double gamma,
                              double intercept, void* ws, int64_t ws_bytes, double* est, void* stream);
/* KNeighborsRegressor(n_neighbors = k).predict on the rows of feat [B][D]: edgedet_knn_fit_predict's distances
 * (the same chain per pair) and its selection rule (the k smallest keys, ties at the k-th distance to the
 * lowest position); est [B] the mean of the selected targets summed in position order, nbr [B][k] (or null)
 * the selected positions ascending.  1 <= k <= n. */
int edgedet_knn_model_predict(const double* feat, int64_t B, int64_t D, const double* mean, const double* scale,
                              const double* z, const double* norm, const double* target, int64_t n, int32_t k,
                              void* ws, int64_t ws_bytes, double* est, int32_t* nbr, void* stream);

/* ------------------------------------------------------------------ gradient boosting regressor (regression.py) */
/*
 * regression.py's GradientBoostingRegressor(learning_rate, n_estimators, subsample = 1.0) with max_depth 1..4
 * and criterion friedman_mse behind fit_model's StandardScaler, every cross-validation fold in flight
 * (csrc/gbr.hip).  The residuals of a stage are carried as integers rq = rint(r 2^q), so every
 * residual sum is exact and a split's gain does not depend on the order of summation; among bit-equal gains
 * the lowest feature wins, then the lowest threshold.  The caller owns every buffer; the launchers allocate
 * nothing, do not synchronise and return -1 with edgedet_last_error set on a bad argument.
 *
 * x, N, D, tr_idx, tr_off_host, tr_off, folds, mean, scale are the estimator regressors' (every fold
 * non-empty, 1 <= D <= 255).  Trees are stored in heap layout (children of node i at 2 i + 1, 2 i + 2):
 * feature int16 [F][T][2^depth - 1] (-1 = leaf), threshold [F][T][2^depth - 1], value [F][T][2^(depth+1) - 1]
 * (0 for a node that does not exist); a row goes right when double(z32) > threshold.
 *
 * edgedet_gbr_workspace_size: bytes of the workspace of edgedet_gbr_fit (and, with folds = 1 and tr_off_host =
 * {0, n}, of edgedet_gbr_best_split); < 0 on bad sizes.  The workspace is 8-byte aligned.
 */
int64_t edgedet_gbr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D);
/* z32 [F][N][D] = float((x - mean_f) / scale_f): a true float64 division, rounded to float32. */
int edgedet_gbr_prepare(const double* x, int64_t N, int64_t D, const double* mean, const double* scale,
                        int32_t folds, float* z32, void* stream);
/* The whole fit, enqueued without a host round trip: per stage one scan launch and one select launch per tree
 * level and one update launch.  y [F][N] the targets; pos [F][N] a row's position in its fold's training list
 * (-1: a validation row); ord and sorted hold per fold f (at tr_off[f] * D) and feature j (at j * n_f) the
 * training positions in the order of z32[:, j] (ties by position) and those values; init [F] = F0, the mean of
 * the training targets; q [F] (host and device) the residual scale, 26 <= q <= 1000.  est [F][N] is the
 * running F of every row and the estimates at the end; nodes [F][T] the split nodes per stage; tied [F] the
 * split nodes with a second feature at the maximal gain; status [F]: 0, or the 1-based stage whose residuals
 * reached 2^(62 - ceil(log2 n)) in magnitude (read it once, after the stream has drained). */
int edgedet_gbr_fit(const float* z32, int64_t N, int64_t D, const double* y, const int32_t* tr_idx,
                    const int32_t* pos, const int32_t* ord, const float* sorted, const int64_t* tr_off_host,
                    const int64_t* tr_off, int32_t folds, const double* init, const int32_t* q_host, const int32_t* q,
                    double learning_rate, int32_t T, int32_t depth, void* ws, int64_t ws_bytes, int16_t* feature,
                    double* threshold, double* value, double* est, int32_t* nodes, int32_t* tied, int32_t* status,
                    void* stream);
/* One level's scan and arg-best of one fold, for a given map node [n] of training positions to nodes (a value
 * >= nn: in no node) and residual quanta rq [n]: per node m < nn (nn = 1, 2, 4 or 8) the best candidate's
 * feature (-1: no valid candidate), threshold, gain, left count wl and left sum Sl, leaf (1 when sklearn's rules
 * other than the depth limit make the node a leaf) and tied (a second feature attains the gain). */
int edgedet_gbr_best_split(const int32_t* ord, const float* sorted, int64_t n, int64_t D, const uint8_t* node,
                           const int64_t* rq, int32_t nn, int32_t q, void* ws, int64_t ws_bytes, int32_t* feature,
                           double* threshold, double* gain, int32_t* wl, int64_t* Sl, int32_t* leaf, int32_t* tied,
                           void* stream);
/* est [B] = init + lr v_1 + lr v_2 + ... of one fold's trees (feature, threshold [T][2^depth - 1], value
 * [T][2^(depth+1) - 1]) on the rows of feat [B][D], standardised as edgedet_gbr_prepare does: the leaf values
 * are gathered in parallel, the sum is formed in stage order with every product and sum rounded by itself, so
 * the estimate equals the fit's bit for bit and does not depend on B. */
int edgedet_gbr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean, const double* scale,
                              const int16_t* feature, const double* threshold, const double* value, double init,
                              double learning_rate, int32_t T, int32_t depth, double* est, void* stream);

/* ------------------------------------------------------------------ random forest regressor (regression.py) */
/*
 * regression.py's RandomForestRegressor(n_estimators, max_depth, min_samples_split) at sklearn's defaults
 * (bootstrap on, every feature tried at every node) behind fit_model's StandardScaler, every tree of every
 * cross-validation fold in flight (csrc/rfr.hip).  The bootstrap of a tree is given as integer row
 * weights w (a row with w = 0 does not exist for that tree), the targets as integers yq = rint((y - F0) 2^q), so
 * every weighted sum is exact and a split's gain does not depend on the order of summation; among bit-equal
 * gains the lowest feature wins, then the lowest threshold.  The caller owns every buffer; the launchers
 * allocate nothing, do not synchronise and return -1 with edgedet_last_error set on a bad argument.
 *
 * x, N, D, tr_idx, tr_off_host, tr_off, folds, mean, scale are the estimator regressors' (every fold non-empty,
 * 1 <= D <= 255); z32, ord and sorted are edgedet_gbr_fit's.  Trees are stored as padded arrays [F][T][cap],
 * cap = edgedet_rfr_node_cap(the largest fold's rows, max_depth) = min(2^(max_depth+1) - 1, 2 n - 1), the nodes
 * numbered breadth first (the children of the split nodes of a level get consecutive ids in parent order, left
 * then right): feature int16 (-1 = leaf or unused), threshold, left int32 (the right child is left + 1; -1 = leaf
 * or unused), value (F0 + (S / W) 2^-q of the node's rows), n_node_samples (in-bag rows); a row goes right when
 * double(z32) > threshold.
 *
 * edgedet_rfr_workspace_size: bytes of the workspace of edgedet_rfr_fit; < 0 on bad sizes.  groups (1..16) is
 * the number of workgroups that share the features of one tree in a scan; no result depends on it.
 * edgedet_rfr_best_split_workspace_size: the same for edgedet_rfr_best_split.  Workspaces are 8-byte aligned.
 */
int64_t edgedet_rfr_node_cap(int64_t n, int32_t max_depth);
int64_t edgedet_rfr_workspace_size(const int64_t* tr_off_host, int32_t folds, int64_t D, int32_t T, int32_t max_depth,
                                   int32_t min_samples_split, int32_t groups);
int64_t edgedet_rfr_best_split_workspace_size(int64_t n, int64_t D, int32_t nn, int32_t groups);
/* The whole fit, enqueued without a host round trip: one root launch, then one scan launch and one select launch
 * per level (a finished tree's workgroups return at once), then one predict launch per fold.  w holds per fold f
 * (at tr_off[f] * T) and tree t (at t * n_f) the weight of every training position; yq (at tr_off[f]) the
 * targets' quanta, |yq| < 2^(62 - ceil(log2 n_f)); init [F] = F0; q [F] (host and device), 26 <= q <= 1000.  est
 * [F][N] = the sum of a row's leaf values in tree order, divided by T; node_count [F][T]; tied [F] the split nodes
 * with a second feature at the maximal gain; status [F] stays 0 (read it once, after the stream has drained). */
int edgedet_rfr_fit(const float* z32, int64_t N, int64_t D, const double* x, const double* mean, const double* scale,
                    const int32_t* tr_idx, const int32_t* ord, const float* sorted, const int64_t* tr_off_host,
                    const int64_t* tr_off, int32_t folds, const double* init, const int32_t* q_host, const int32_t* q,
                    const uint8_t* w, const int64_t* yq, int32_t T, int32_t max_depth, int32_t min_samples_split,
                    int32_t groups, void* ws, int64_t ws_bytes, int16_t* feature, double* threshold, int32_t* left,
                    double* value, int32_t* n_node_samples, int32_t* node_count, int32_t* tied, int32_t* status,
                    double* est, void* stream);
/* One level's scan and arg-best of one tree, for a given map slot [n] of training positions to nodes (a value
 * outside 0..nn-1: in no node), weights w [n] and quanta yq [n]: per node m < nn its in-bag rows cnt, weighted
 * count W and sum S, the best candidate's feature (-1: no valid candidate), threshold, gain, left weighted count
 * wl, left rows cl and left sum Sl, leaf (1 when sklearn's rules other than the depth limit make the node a leaf)
 * and tied (a second feature attains the gain). */
int edgedet_rfr_best_split(const int32_t* ord, const float* sorted, int64_t n, int64_t D, const int32_t* slot,
                           const uint8_t* w, const int64_t* yq, int32_t nn, int32_t q, int32_t min_samples_split,
                           int32_t groups, void* ws, int64_t ws_bytes, int32_t* cnt, int32_t* W, int64_t* S,
                           int32_t* feature, double* threshold, double* gain, int32_t* wl, int32_t* cl, int64_t* Sl,
                           int32_t* leaf, int32_t* tied, void* stream);
/* est [B] of one fold's forest (arrays [T][cap]) on the rows of feat [B][D], standardised as edgedet_gbr_prepare
 * does: one thread per (row, tree) walks the tree, one thread per row adds the leaf values in tree order and
 * divides by T, so the estimate equals the fit's bit for bit and does not depend on B. */
int edgedet_rfr_model_predict(const double* feat, int64_t B, int64_t D, const double* mean, const double* scale,
                              const int16_t* feature, const double* threshold, const int32_t* left,
                              const double* value, int32_t T, int64_t cap, double* est, void* stream);

/* ------------------------------------------------------------------ offloading cascade (csrc/offload.hip) */
/*
 * The on-device decision chain between the weak and the strong detector (edgeml_amd.offload); every
 * call is asynchronous on `stream` and the caller owns every buffer.
 *
 * edgedet_offload_rows: detect.py:79-105 on a plan's raw outputs count [B], boxes [B][K][4], scores
 * [B][K], labels [B][K] of H x W images: rows [B][K][6] float64 [cls, xc, yc, w, h, conf], each image's
 * kept rows (coco: the COCO-91 -> YOLO-80 map without the 11 dropped ids, an id outside 0..90 dropped
 * too; voc != 0: label - 1, label 0 dropped) compacted to the front in score order, nrow [B] their
 * count.  The first nrow rows are byte-identical to numpy's float32 arithmetic promoted to float64; the
 * rows past them are not written.
 */
int edgedet_offload_rows(const int32_t* count, const float* boxes, const float* scores, const int64_t* labels,
                         int64_t B, int64_t K, int32_t H, int32_t W, int32_t voc, double* rows, int32_t* nrow,
                         void* stream);
/* edgedet_output_features on padded rows [B][K][6] with nrow [B] kept rows each: out [B][num_class + 5 k],
 * byte-identical to it (counts over the first min(nrow, k) rows, int(cls) truncated, zeros beyond). */
int edgedet_offload_features(const double* rows, const int32_t* nrow, int64_t B, int64_t K, int32_t num_class,
                             int32_t k, double* out, void* stream);
/*
 * est [B] = the estimator on feat [B][D], flag [B] = est > threshold (strict, test.py:37).  L = 0: a
 * linear model, est by edgedet_reg_predict (folds = 1; mean, scale, coef [D] and intercept [1] on the
 * device).  L >= 1: an MLP of L linear layers (dims on the host, state on the device, as
 * edgedet_mlp_predict takes them): feat is cast to float32 into x32 [B][D], est32 [B] comes from
 * edgedet_mlp_predict and est is its promotion to float64.  The estimates are those two exports' bit for
 * bit: their kernels run unchanged.
 */
int edgedet_offload_decide(const double* feat, int64_t B, int64_t D, const double* mean, const double* scale,
                           const double* coef, const double* intercept, int32_t L, const int32_t* dims,
                           const float* state, float* x32, float* est32, double threshold, double* est,
                           uint8_t* flag, void* stream);
/* flag [B] = est [B] > threshold (strict, float64): edgedet_offload_decide's last step on estimates another
 * call wrote (edgedet_svr_model_predict, edgedet_knn_model_predict); the same kernel, est is only read. */
int edgedet_offload_flag(const double* est, int64_t B, double threshold, uint8_t* flag, void* stream);
/*
 * The DCSB baseline's decision (baseline.py:129-141) for one fitted model (conf_thresh, num_thresh, area_thresh)
 * on the padded rows of edgedet_offload_rows.  Per image b, over its first clamp(nrow[b], 0, K) rows r:
 * conf = r[5]; x1 = r[1] - r[3]/2, y1 = r[2] - r[4]/2, x2 = r[1] + r[3]/2, y2 = r[2] + r[4]/2 and
 * area = (x2 - x1) * (y2 - y1) (xywh2xyxy then get_area, each op rounded on its own);
 * est_num = #(conf > conf_thresh), det_num = #(conf > 0.5), min_area = the minimum area among the rows with
 * conf > conf_thresh (0.0 when there are none; a NaN area wins, as np.amin);
 * cls = est_num != det_num && (est_num > num_thresh || min_area < area_thresh); est[b] = cls ? 1.0 : 0.0 and
 * flag[b] = cls.  Every comparison is strict and the rows at or past nrow[b] are never read.  est_num, det_num
 * and min_area [B] are optional (null: not written).  float64 and integers only; one wave per image, nothing
 * allocated.  B <= 65535 (B == 0: no launch), 1 <= K < 2^24.
 */
int edgedet_offload_dcsb(const double* rows, const int32_t* nrow, int64_t B, int64_t K, double conf_thresh,
                         int32_t num_thresh, double area_thresh, int32_t* est_num, int32_t* det_num,
                         double* min_area, double* est, uint8_t* flag, void* stream);
/*
 * The Adaptive Feeding baseline's decision on feat [B][D] (edgedet_offload_features' output): v [Dp] is the
 * SVM's coef [D], its intercept at index D, then zeros, Dp = (D + 1 + 15) / 16 * 16 <= 256 (anything else is
 * refused): baseline.pad_features' layout with the padding implied, no padded copy of the features is read.
 * est[b] is, bit for bit, what edgedet_svm_decision gives for row b of pad_features(feat) with that v (sixteen
 * lanes per row, a lane's terms in increasing k, then the 8-4-2-1 butterfly); flag[b] = est[b] > 0 (strict).
 * B <= 65535 (B == 0: no launch).
 */
int edgedet_offload_svm(const double* feat, int64_t B, int64_t D, const double* v, int64_t Dp, double* est,
                        uint8_t* flag, void* stream);
/* The images b of src [B][image_bytes] with flag[b] != 0 copied to the front of dst in index order
 * (flags read on the device); *count their number, index[0 .. count) their source indices.  16-byte
 * copies where an image's two ends are 16-byte aligned, bytes otherwise and for the tail.  Nothing is
 * written past the count-th image or index. */
int edgedet_offload_pack(const uint8_t* flag, const uint8_t* src, int64_t B, int64_t image_bytes, uint8_t* dst,
                         int32_t* count, int32_t* index, void* stream);
/* dst [n_images][image_bytes]: image j is image index[j] of the device batch src[j] (1 <= n_images <= 64;
 * src and index are host arrays, passed to the kernel by value). */
int edgedet_offload_gather(const void* const* src, const int32_t* index, int32_t n_images, int64_t image_bytes,
                           uint8_t* dst, void* stream);

/* ------------------------------------------------------------------ image ingest (read_image) */
/*
 * torchvision.io.read_image(path, ImageReadMode.RGB) of detect.py:55-58 for baseline JPEGs, split
 * host / device (csrc/jpeg.hip): edgedet_jpeg_packet entropy-decodes one file's bytes on the calling
 * host thread into a packet (the nonzero coefficients of every 8x8 block + the quantisation tables);
 * returns its size (written to out when cap suffices; hw = {H, W}), 0 for a JPEG it does not handle
 * (progressive, arithmetic, CMYK/RGB, other samplings: decode that file on the host), < 0 on corrupt
 * data.  edgedet_jpeg_decode_batch runs dequantisation + islow IDCT + fancy upsampling + YCbCr->RGB for
 * B packets of one H x W already on the device (packets + offsets[b]) into out [B][3][H][W] uint8,
 * byte-identical to libjpeg's default decode; planes: B * plane_stride bytes of scratch,
 * plane_stride >= max_blocks * 64 = the largest edgedet_jpeg_plane_bytes of the batch.
 * edgedet_jpeg_reconstruct_host is the same reconstruction on the host (test checker).
 */
int64_t edgedet_jpeg_packet(const uint8_t* data, int64_t size, void* out, int64_t cap, int32_t* hw);
/* A batch of n JPEG files entropy-decoded on `threads` host threads (0 = all) straight into the device
 * image edgedet_jpeg_decode_batch reads (offsets = packets = out once uploaded): out[0..8n) the int64
 * packet offsets (padded to 256 B), then the 256-B aligned packets; hw[2i..2i+1] = (H, W) of file i,
 * *max_plane_bytes = the largest plane_bytes of the batch.  Returns the span to upload; a span above
 * cap means nothing usable was written (retry with that many bytes).  0 = a file the device path does
 * not handle (decode the batch on the host), < 0 = unreadable or corrupt file.  The detect CLI's image
 * read (detect.py:55-58) for one batch in one call. */
int64_t edgedet_jpeg_batch_packets(const char* const* paths, int64_t n, void* out, int64_t cap, int32_t* hw,
                                   int64_t* max_plane_bytes, int32_t threads);
/* (H, W) of n image files from their headers (JPEG SOFn, PNG IHDR; what PIL's Image.open(path).size
 * reports, the shapes read_image returns), parsed on `threads` host threads (0 = all): hw[2i], hw[2i+1];
 * (0, 0) for a file whose header was not understood (the caller falls back).  Returns the count found. */
int64_t edgedet_image_dims(const char* const* paths, int64_t n, int32_t* hw, int32_t threads);
int64_t edgedet_jpeg_plane_bytes(const void* host_packet);
int edgedet_jpeg_decode_batch(const void* packets, const int64_t* offsets, int32_t B, int32_t H, int32_t W,
                              int32_t max_blocks, void* planes, int64_t plane_stride, uint8_t* out, void* stream);
int edgedet_jpeg_reconstruct_host(const void* host_packet, uint8_t* out);

/* ------------------------------------------------- conv-stack estimator (csrc/convnet.hip) */
/*
 * The kernels of one training step of lib/nn_model.py EdgeDetectionNet with conv stacks
 * (regression.py:242-355 fit_CNN on the hidden-layer feature maps; the host loop is edgeml_amd/convnet.py,
 * DESIGN.md 6g).  Everything is NHWC: a map [B][H][W][C] and a batch [B][D] are both a matrix [M][C] of
 * M rows (pixels or samples) by C channels.  The conv forward and data gradient are edgedet_conv2d_ex.
 * No kernel uses atomics: every result is bit-identical from run to run.
 *
 * edgedet_cnn_wgrad: dw[co][kh][kw][ci] = sum_{b,h,w} dy[b][h][w][co] x[b][h+kh-k/2][w+kw-k/2][ci] (zero
 *   outside the map) for a stride-1 'same' conv of odd size k, on v_mfma_f32_16x16x4_f32 with K = B*H*W
 *   summed in stages of 64 pixels.  dw is dense [Cout][k*k*Cin] (no row padding).
 * edgedet_cnn_repack: w [Cout][k][k][Cin] dense -> wf [Cout][edgedet_conv_weight_k(k, k, Cin)], the conv
 *   engine's forward pack, and (wb non-null) wb [Cin][edgedet_conv_weight_k(k, k, Cout)] =
 *   w[co][k-1-kh][k-1-kw][ci] at [ci][kh][kw][co], the pack whose conv over dy is the data gradient.
 *   Only the weights are written: the caller zeroes the row pads once.
 * edgedet_cnn_bn_stats: BatchNorm (1d or 2d) train statistics of z [M][C]: mean, invstd =
 *   1 / sqrt(biased var + 1e-5), and running = 0.9 running + 0.1 (mean | unbiased var).
 * edgedet_cnn_act_fwd: a = dropout(relu(gamma h + beta)); mode 0: h = z (no BatchNorm, gamma / beta unused);
 *   mode 1: h = (z - mean) invstd; mode 2 (eval): mean / invstd point at the running mean / running VAR.
 *   xhat (nullable) receives h.  Dropout (dropout > 0): element (row r = b HW + pix, channel c) is kept when
 *   u >= dropout for u = the top 24 bits of splitmix64(key, step << 32 | ((b C + c) HW + pix)), i.e. the
 *   counter is the element's NCHW flat index, independent of the device layout; kept values are scaled by
 *   1 / (1 - dropout).  key = seed ^ fold << 48 ^ layer << 40 by convention (edgeml_amd/convnet.py).
 * edgedet_cnn_col_reduce: a null: out0[c] = sum_r v[r][c] (a bias gradient).  a non-null: v is the
 *   gradient behind ReLU + Dropout, dy = a > 0 ? v scale : 0; out0 = sum dy (dbeta), out1 = sum dy xhat (dgamma).
 * edgedet_cnn_act_bwd: dz = bn ? (dy - sdy / M - xhat sdyx / M) invstd gamma : dy with dy as above.
 * edgedet_cnn_maxpool_fwd / _bwd: MaxPool2d(2, 2), floor mode; idx [B][H/2][W/2][C] holds h W + w of the
 *   first maximum in window order (torch's argmax); the backward routes dy to it, zero elsewhere.
 * edgedet_cnn_gmean_fwd / _bwd: mean over the HW pixels of x [B][HW][C] and its gradient.
 * edgedet_cnn_linear_fwd: z [B][dout] = x [B][din] w[dout][din]^T + bias; _dx: dx = dz w.
 * edgedet_cnn_loss: loss[0] = mean (pred - y)^2 (times y when weighted); dpred (nullable) its gradient.
 * edgedet_cnn_adam: torch.optim.Adam's single-tensor step over n parameters: step_size = lr / (1 - 0.9^t)
 *   and bc2_sqrt = sqrt(1 - 0.999^t) computed by the caller in double.
 */
int edgedet_cnn_wgrad(const float* x, const float* dy, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                      int32_t k, float* dw, void* stream);
int edgedet_cnn_repack(const float* w, int64_t Cout, int64_t Cin, int32_t k, float* wf, float* wb, void* stream);
int edgedet_cnn_bn_stats(const float* z, int64_t M, int64_t C, float* running_mean, float* running_var, float* mean,
                         float* invstd, void* stream);
int edgedet_cnn_col_reduce(const float* v, const float* a, const float* xhat, int64_t M, int64_t C, float scale,
                           float* out0, float* out1, void* stream);
int edgedet_cnn_act_fwd(const float* z, int64_t M, int64_t C, int64_t HW, const float* gamma, const float* beta,
                        const float* mean, const float* invstd, int32_t mode, float dropout, uint64_t key,
                        uint64_t step, float* xhat, float* a, void* stream);
int edgedet_cnn_act_bwd(const float* da, const float* a, const float* xhat, int64_t M, int64_t C, float scale,
                        const float* gamma, const float* invstd, const float* sdy, const float* sdyx, int32_t bn,
                        float* dz, void* stream);
int edgedet_cnn_maxpool_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, int32_t* idx,
                            void* stream);
int edgedet_cnn_maxpool_bwd(const float* dy, const int32_t* idx, int64_t B, int64_t H, int64_t W, int64_t C,
                            float* dx, void* stream);
int edgedet_cnn_gmean_fwd(const float* x, int64_t B, int64_t HW, int64_t C, float* y, void* stream);
int edgedet_cnn_gmean_bwd(const float* dy, int64_t B, int64_t HW, int64_t C, float* dx, void* stream);
int edgedet_cnn_linear_fwd(const float* x, int64_t B, int64_t din, int64_t dout, const float* w, const float* bias,
                           float* z, void* stream);
int edgedet_cnn_linear_dx(const float* dz, int64_t B, int64_t din, int64_t dout, const float* w, float* dx,
                          void* stream);
int edgedet_cnn_loss(const float* pred, const float* y, int64_t n, int32_t weighted, float* loss, float* dpred,
                     void* stream);
int edgedet_cnn_adam(float* param, const float* grad, float* m, float* v, int64_t n, float step_size, float bc2_sqrt,
                     float weight_decay, void* stream);

/* ------------------------- the cascade's decision from a hidden-layer map (csrc/tapnet.hip, csrc/lower.hip) */
/*
 * edgedet_ssdlite_taps: the stage table of the SSDLite plan of (num_classes, reduced_tail, B, H, W, input_u8).
 *   Stage N is the output of torchvision's mobilenet_v3_large.features[N] (1-15: the InvertedResidual blocks,
 *   token "IR"; 16: the last 1x1 conv, "Conv"; 0: the stem conv, "Conv") and stages 17-20 are backbone.extra.0-3
 *   ("Extra").  Every batch chain of the plan has a tap per stage: the workspace buffer [images][H][W][C] that
 *   holds the stage's output for the chain's images [image0, image0 + images) of the batch.  stage >= 0: the
 *   taps of that stage, one per chain in chain order; stage = -1: every tap, by stage then chain.  Returns the
 *   count and fills out[] when cap is large enough; -1 (edgedet_last_error) for a stage outside the table, and
 *   for stage 0 under the fused stem (EDGEDET_SSD_STEM_FUSE=1, the default), where the stem conv's output never
 *   reaches memory.
 */
typedef struct edgedet_tap {
    int32_t stage;
    int32_t chain;
    char token[8];    /* the file-name token: stage{N}_{token}_features.npy */
    char buffer[96];  /* the workspace buffer's name (edgedet_model_buffers) */
    int64_t image0, images, C, H, W;
} edgedet_tap;
int64_t edgedet_ssdlite_taps(int32_t num_classes, int32_t reduced_tail, int32_t B, int32_t H, int32_t W,
                             int32_t input_u8, int32_t stage, edgedet_tap* out, int64_t cap);
/*
 * The eval-mode forward of edgeml_amd.convnet's conv-stack net (resize on) as one launch, one workgroup per
 * image: x [B][S][S][cin] the pooled maps, `channels` / `kernels` / `pools` [nconv] the conv layers (output
 * channels, odd kernel size, 1 = MaxPool 2x2 after it), dims [nlin + 1] the linear widths (dims[0] = the
 * flattened last map, dims[nlin] = 1), state [ns] the net's state vector in ConvSpec's layout.  Writes
 * est[b] = (double) the float32 estimate and flag[b] = est[b] > threshold (strict, as edgedet_offload_flag).
 * Conv layers are implicit GEMMs on v_mfma_f32_16x16x4_f32 with K = (kh, kw, ci) ascending in one chain per
 * output; BatchNorm is cnn_act_fwd's mode 2; linear sums are edgedet_cnn_linear_fwd's.  No atomics: an
 * image's estimate does not depend on the batch it runs in.
 * edgedet_tapnet_fits: 1 when the net is inside the kernel's domain (kernels.hpp tapnet_fits: the activation
 *   planes' two LDS regions within 160 KiB, channel counts multiples of 4, odd kernels), else 0;
 *   edgedet_tapnet_lds: the bytes of those regions (-1: not a net).  edgedet_tapnet_infer returns
 *   EDGEDET_TAPNET_NOFIT for a net outside the domain, before it looks at any pointer.
 * edgedet_tapnet_finish: est = (double) est32, flag = est > threshold: the tail of the layered eval forward.
 */
#define EDGEDET_TAPNET_NOFIT (-4)
int edgedet_tapnet_fits(int32_t S, int32_t cin, int32_t nconv, const int32_t* channels, const int32_t* kernels,
                        const int32_t* pools, int32_t nlin, const int32_t* dims);
int64_t edgedet_tapnet_lds(int32_t S, int32_t cin, int32_t nconv, const int32_t* channels, const int32_t* kernels,
                           const int32_t* pools, int32_t nlin, const int32_t* dims);
int edgedet_tapnet_infer(const float* x, int64_t B, int32_t S, int32_t cin, int32_t nconv, const int32_t* channels,
                         const int32_t* kernels, const int32_t* pools, int32_t nlin, const int32_t* dims,
                         const float* state, int64_t ns, double threshold, double* est, uint8_t* flag, void* stream);
int edgedet_tapnet_finish(const float* est32, int64_t B, double threshold, double* est, uint8_t* flag, void* stream);

/* --------------------------------------------------------------------------------- misc */
const char* edgedet_last_error(void);
/* Library/ABI version: (major << 16) | minor. */
int32_t edgedet_version(void);
/* Device code target the library was built for ("gfx950"). */
const char* edgedet_target(void);

#ifdef __cplusplus
}
#endif
#endif /* EDGEDET_H */
