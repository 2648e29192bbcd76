// The field layout of every edgedet_op record kind (include/edgedet.h): which slot of i[] (int64),
// p[] (device pointers), f[] (floats) and d[] (doubles) holds what.  The lowering (lower.hip) writes
// records and the executor (exec.hip) reads them through these names only; the values are frozen (the
// Python host and the tests index records by number).
//
// One namespace per kind, one plain enum per array the kind uses (I, P, F, D).  "| 0" marks an optional
// pointer (null = absent).  A name ending in 0 is the base of a per-level run, used as `base + l`.
// i[EDGEDET_OP_LANE] (edgedet.h) of every record is its lane.
#pragma once

namespace edgedet::rec {

// The five pointers of a record list (what SegOut holds), in order from a kind's `records0` base:
// per segment up to kmax kept boxes, their scores, merge tiebreaks and labels, and the count.
namespace seg {
enum { box, score, tb, label, count };
}

namespace mem_set {
enum I { bytes };
enum P { ptr };
}

// GeneralizedRCNNTransform: exactly one of x / xu8 is set.
namespace preprocess {
enum I { B, H, W, Ho, Wo, Hp, Wp };  // source size, resized size, padded size
enum P {
    x,    // [B,3,H,W] f32 | 0
    y,    // [B,Hp,Wp,4]
    xu8,  // [B,3,H,W] u8 | 0
};
enum F { mean0 = 0, std0 = 3 };  // + channel
}

namespace conv {
enum I {
    B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, act,
    K, Kpad,
    x_pstride, y_pstride, res_pstride,  // pixel strides (elements)
    x_bstride, y_bstride, res_bstride,  // batch strides (elements)
    y_off,                              // element offset into y
    res_H, res_W,                       // nearest-upsample source of the residual, 0 = same as the output
    tile,                               // ConvTile (kernels.hpp), 0 = auto
    in_relu,
};
enum P {
    x,
    w,         // [Cout][Kpad]
    bias,
    y,
    res,       // | 0
    in_scale,  // [B][Cin] | 0
    w3,        // bf16 planes [3][Cout][Kpad] | 0
    in_shift,  // [B][Cin] | 0
    x3,        // scratch [3][B*H*W*Cin] bf16 | 0: pre-split input planes for the 256 x 128 bf16x6 tile (the
               // split and the input transform run once per input element instead of once per N tile)
    stamp,     // timing probe slot (2 x u64; bf16x6 tiles only) | 0; 0 in product plans
};
}

// SSDLite features.0.0 + features.0.1 fused, the transform folded into the stem's loads.
namespace ssd_stem {
enum I {
    B, H, W, Ho, Wo,  // H x W: the stem conv's input (the resized image)
    ld0, ld1,         // row lengths of w0 / w1
    H0, W0,           // source image size
};
enum P {
    x,  // NHWC4 (unused when src / src8 is set)
    w0,  // [16][ld0]
    b0,
    wd,  // [9][16]
    bd,
    w1,  // [16][ld1]
    b1,
    y,
    src,   // [B,3,H0,W0] f32 | 0
    src8,  // [B,3,H0,W0] u8 | 0
};
enum F { mean0 = 0, std0 = 3 };  // + channel
}

namespace dwconv {
enum I { B, H, W, C, Ho, Wo, K, stride, pad, act, parts };  // parts: SE partial-sum splits (0 = 16)
enum P {
    x,
    w,     // [K*K][C]
    bias,
    y,
    part,  // SE partial sums [B,parts,C] | 0
};
}

// InvertedResidual without SE in one kernel.
namespace mbconv {
enum I { B, H, W, Cin, Cexp, Cout, Ho, Wo, K, stride, pad, act, ld1, ld2, residual };
enum P {
    x,
    w1,  // expand [Cexp][ld1]
    b1,
    wd,  // depthwise [K*K][Cexp]
    bd,
    w2,  // project [Cout][ld2]
    b2,
    y,
};
}

namespace channel_mean {
enum I { B, HW, C };
enum P { x /* [B,HW,C] */, mean /* [B,C] */ };
}

namespace se_fc {
enum I { B, C, S, HW, parts };  // parts: 0 = 16
enum P {
    part,    // [B,parts,C]
    w1,      // [S][C]
    b1,
    w2t,     // [S][C]
    b2,
    scale,   // [B,C]
    hidden,  // [B,S]
};
}

namespace maxpool {
enum I { B, H, W, C, Ho, Wo, K, stride, pad };
enum P { x, y };
}

namespace ssd_scores {
enum I { B, A, NC };
enum P {
    logits,    // [B,A,NC]
    reg,       // [B,A,4]
    anchors,   // [A,4]
    scores_t,  // [B,NC,A]
    boxes,     // [B,A,4]
};
enum F { img_h, img_w };
}

namespace ssd_class_nms {
enum I { B, A, NC, topk, kmax };
enum P { scores_t, boxes, records0 };  // records0 + seg::*
enum F { score_thresh };
enum D { iou };
}

namespace merge_topk {
enum I { B, S, kmax, N };
enum P {
    records0 = 0,  // + seg::*
    ratio = 5,     // [B,2] | 0
    out_box,
    out_score,
    out_label,  // | 0
    out_count,
};
}

namespace rpn_level_nms {
enum I {
    B, nlevels,
    ld,  // unused
    A, topk, kmax,
    n0 = 6,  // + level: anchors of the level
    chunk = 16, nchunk,
};
enum P {
    obj0 = 0,       // + level: objectness [B][n]
    anchors0 = 5,   // + level
    records0 = 10,  // + seg::*
    deltas0 = 15,   // + level: [B][n][4]
    ckey = 20,      // chunked top-k (optional): | 0
    cidx,           // [B,levels,nchunk,1024]
    ccount,         // [B,levels,nchunk]
    split,          // split NMS scratch [rpn_split_bytes(B * levels)] | 0
};
enum F { img_h, img_w, min_size, score_thresh };
enum D { iou };
}

namespace roi_align {
enum I { mode, R, RMAX, B, C, PH, PW, sr, nlevels, k_min, k_max, H0 = 11, W0 = 15 };  // H0 / W0 + level
enum P { feat0 = 0 /* + level */, rois = 4, counts, out };
enum F { scale0 };  // + level
}

namespace box_scores {
enum I { ld, B, R, NC, cls_off, delta_off };
enum P { pred, props, counts, scores, boxes };
enum F { img_h, img_w };
}

namespace box_class_nms {
enum I { B, R, NC, kmax };
enum P { scores, boxes, counts, records0 };  // records0 + seg::*
enum F { score_thresh, min_size };
enum D { iou };
}

namespace ssd_postprocess {
enum I { B, A, NC, topk, N, select_wave };  // select_wave: 1 = one-wave class select
enum P {
    scores_t,
    boxes,
    pool_key,
    pool_ref,
    ratio,  // | 0
    out_box,
    out_score,
    out_label,  // | 0
    out_count,
};
enum F { score_thresh };
enum D { iou };
}

namespace gn_stats {
enum I { B, HW, C, G };
enum P { x /* [B,HW,C] */, gamma, beta, scale /* [B,C] */, shift /* [B,C] */ };
enum F { eps };
}

namespace retina_select {
enum I {
    B, L, Atot, K, topk, kmax,
    first0 = 6,   // + level: the level's first anchor
    count0 = 11,  // + level: anchors of the level
    chunk = 16, nchunk,
};
enum P {
    logits,        // [B,Atot,K]
    deltas,        // [B,Atot,4]
    anchors,       // [Atot,4]
    records0 = 3,  // + seg::*, [B,L,kmax]
    ckey = 8,      // chunk scratch: keys,
    cidx,          // flat indices [B,L,nchunk,1024],
    ccount,        // counts [B,L,nchunk]
};
enum F { img_h, img_w, score_thresh };
}

namespace retina_class_nms {
enum I { B, L, kin, K, kmax };
enum P { level0 = 0, records0 = 5 };  // + seg::*: level records in, class records [B,K,kmax] out
enum D { iou };
}

namespace fork {  // side lanes 1..lanes wait for lane 0
enum I { lanes };
}
namespace join {  // lane 0 waits for side lanes 1..lanes
enum I { lanes };
}
namespace wait {  // lane `waiter` waits for everything issued so far on lane `waited` (both forked, or 0)
enum I { waiter, waited };
}
namespace group {  // the next `members` records as one grouped launch
enum I { members };
}

}  // namespace edgedet::rec
