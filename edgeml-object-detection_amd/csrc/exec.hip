// Native plan executor of libedgedet.so.
//
// A detector forward is lowered by the Python host (edgeml_amd/plan.py) into a flat array of
// edgedet_op records; this file decodes each record into its kernel's parameter block and launches
// it on the caller's stream, or captures the whole sequence once into a hipGraph that is replayed
// per batch (one host call per forward; no allocation, no sync, no host round trip inside).
//
// Record layouts (which slot of i / p / f / d holds what, per kind): csrc/records.hpp.
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>
#include <string>

#include <map>
#include <set>
#include <utility>

#include "kernels.hpp"
#include "records.hpp"

namespace edgedet {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* get_error() { return g_error.c_str(); }

template <typename T>
static T* P(const edgedet_op& o, int k) {
    return reinterpret_cast<T*>(static_cast<uintptr_t>(o.p[k]));
}

// The record list whose five pointers start at slot k0 (a kind's records0, rec::seg order).
static SegOut seg_out(const edgedet_op& o, int k0, int kmax) {
    SegOut s;
    s.box = P<f32x4>(o, k0 + rec::seg::box);
    s.score = P<float>(o, k0 + rec::seg::score);
    s.tb = P<uint32_t>(o, k0 + rec::seg::tb);
    s.label = P<int>(o, k0 + rec::seg::label);
    s.count = P<int>(o, k0 + rec::seg::count);
    s.kmax = kmax;
    return s;
}

// CONV record -> ConvParams.
static ConvParams conv_params(const edgedet_op& o) {
    namespace r = rec::conv;
    const int64_t* I = o.i;
    ConvParams p{};
    p.x = P<const float>(o, r::x);
    p.w = P<const float>(o, r::w);
    p.bias = P<const float>(o, r::bias);
    p.y = P<float>(o, r::y);
    p.res = P<const float>(o, r::res);
    p.in_scale = P<const float>(o, r::in_scale);
    p.w3 = P<const void>(o, r::w3);
    p.in_shift = P<const float>(o, r::in_shift);
    p.in_relu = (int)I[r::in_relu];
    p.x3 = P<void>(o, r::x3);
    p.stamp = P<unsigned long long>(o, r::stamp);
    p.B = (int)I[r::B];
    p.H = (int)I[r::H];
    p.W = (int)I[r::W];
    p.Cin = (int)I[r::Cin];
    p.Ho = (int)I[r::Ho];
    p.Wo = (int)I[r::Wo];
    p.Cout = (int)I[r::Cout];
    p.KH = (int)I[r::KH];
    p.KW = (int)I[r::KW];
    p.stride = (int)I[r::stride];
    p.pad = (int)I[r::pad];
    p.act = (int)I[r::act];
    p.K = (int)I[r::K];
    p.Kpad = (int)I[r::Kpad];
    p.x_pstride = (int)I[r::x_pstride];
    p.y_pstride = (int)I[r::y_pstride];
    p.res_pstride = (int)I[r::res_pstride];
    p.x_bstride = I[r::x_bstride];
    p.y_bstride = I[r::y_bstride];
    p.res_bstride = I[r::res_bstride];
    p.y_off = I[r::y_off];
    p.res_H = (int)I[r::res_H];
    p.res_W = (int)I[r::res_W];
    p.M = p.B * p.Ho * p.Wo;
    return p;
}

// DWCONV record -> DwParams.
static DwParams dw_params(const edgedet_op& o) {
    namespace r = rec::dwconv;
    const int64_t* I = o.i;
    DwParams p{};
    p.x = P<const float>(o, r::x);
    p.w = P<const float>(o, r::w);
    p.bias = P<const float>(o, r::bias);
    p.y = P<float>(o, r::y);
    p.part = P<float>(o, r::part);
    p.B = (int)I[r::B];
    p.H = (int)I[r::H];
    p.W = (int)I[r::W];
    p.C = (int)I[r::C];
    p.Ho = (int)I[r::Ho];
    p.Wo = (int)I[r::Wo];
    p.K = (int)I[r::K];
    p.stride = (int)I[r::stride];
    p.pad = (int)I[r::pad];
    p.act = (int)I[r::act];
    p.parts = I[r::parts] > 0 ? (int)I[r::parts] : SE_PARTS;
    return p;
}

// Diagnostic only (wrong results), compiled in only with -DEDGEDET_DIAG (never in the product
// library): EDGEDET_DIAG_SKIP=k1,k2,... launches nothing for ops of those kinds (100 + t: convs whose
// requested tile is t), to measure what each op family costs the steady-state step under stream
// concurrency.
#ifdef EDGEDET_DIAG
static const uint64_t* diag_skip_masks() {
    static uint64_t m[2] = {0, 0};
    static const bool once = [] {
        uint64_t* w = m;
        if (const char* e = std::getenv("EDGEDET_DIAG_SKIP"))
            for (const char* q = e; *q;) {
                char* end;
                const long k = std::strtol(q, &end, 10);
                if (end == q) break;
                if (k > 0 && k < 64) w[0] |= 1ull << k;
                if (k >= 100 && k < 164) w[1] |= 1ull << (k - 100);
                q = *end ? end + 1 : end;
            }
        return true;
    }();
    (void)once;
    return m;
}
static uint64_t diag_skip_mask() { return diag_skip_masks()[0]; }
#else
static const uint64_t* diag_skip_masks() {
    static const uint64_t m[2] = {0, 0};
    return m;
}
static uint64_t diag_skip_mask() { return 0; }
#endif

static int run_op(const edgedet_op& o, hipStream_t s) {
    const int64_t* I = o.i;
    if ((diag_skip_mask() >> (o.kind & 63)) & 1 && o.kind != EDGEDET_OP_FORK && o.kind != EDGEDET_OP_JOIN) return 0;
    switch (o.kind) {
        case EDGEDET_OP_MEMSET: {
            namespace r = rec::mem_set;
            EDGEDET_CHECK_HIP(hipMemsetAsync(P<void>(o, r::ptr), 0, (size_t)I[r::bytes], s));
            return 0;
        }
        case EDGEDET_OP_PREPROCESS: {
            namespace r = rec::preprocess;
            PreParams p{};
            p.x = P<const float>(o, r::x);
            p.y = P<float>(o, r::y);
            p.xu8 = P<const uint8_t>(o, r::xu8);
            p.B = (int)I[r::B];
            p.H = (int)I[r::H];
            p.W = (int)I[r::W];
            p.Ho = (int)I[r::Ho];
            p.Wo = (int)I[r::Wo];
            p.Hp = (int)I[r::Hp];
            p.Wp = (int)I[r::Wp];
            for (int c = 0; c < 3; ++c) {
                p.mean[c] = o.f[r::mean0 + c];
                p.stdv[c] = o.f[r::std0 + c];
            }
            return preprocess_launch(p, s);
        }
        case EDGEDET_OP_MBCONV: {
            namespace r = rec::mbconv;
            MbParams p{};
            p.x = P<const float>(o, r::x);
            p.w1 = P<const float>(o, r::w1);
            p.b1 = P<const float>(o, r::b1);
            p.wd = P<const float>(o, r::wd);
            p.bd = P<const float>(o, r::bd);
            p.w2 = P<const float>(o, r::w2);
            p.b2 = P<const float>(o, r::b2);
            p.y = P<float>(o, r::y);
            p.B = (int)I[r::B];
            p.H = (int)I[r::H];
            p.W = (int)I[r::W];
            p.Cin = (int)I[r::Cin];
            p.Cexp = (int)I[r::Cexp];
            p.Cout = (int)I[r::Cout];
            p.Ho = (int)I[r::Ho];
            p.Wo = (int)I[r::Wo];
            p.K = (int)I[r::K];
            p.stride = (int)I[r::stride];
            p.pad = (int)I[r::pad];
            p.act = (int)I[r::act];
            p.ld1 = (int)I[r::ld1];
            p.ld2 = (int)I[r::ld2];
            p.residual = (int)I[r::residual];
            return mbconv_launch(p, s);
        }
        case EDGEDET_OP_CONV: {
            const int tile = (int)I[rec::conv::tile];
            if ((diag_skip_masks()[1] >> (tile & 63)) & 1) return 0;
            const ConvParams p = conv_params(o);
            EDGEDET_REQUIRE(p.K == p.KH * p.KW * p.Cin, "conv: K != KH*KW*Cin");
            return conv_launch(p, tile, s);
        }
        case EDGEDET_OP_DWCONV:
            return dwconv_launch(dw_params(o), s);
        case EDGEDET_OP_CHANNEL_MEAN: {
            namespace r = rec::channel_mean;
            return channel_mean_launch(P<const float>(o, r::x), P<float>(o, r::mean), (int)I[r::B], (int)I[r::HW],
                                       (int)I[r::C], s);
        }
        case EDGEDET_OP_SE_FC: {
            namespace r = rec::se_fc;
            return se_fc_launch(P<const float>(o, r::part), P<const float>(o, r::w1), P<const float>(o, r::b1),
                                P<const float>(o, r::w2t), P<const float>(o, r::b2), P<float>(o, r::hidden),
                                P<float>(o, r::scale), (int)I[r::B], (int)I[r::C], (int)I[r::S], (int)I[r::HW],
                                I[r::parts] > 0 ? (int)I[r::parts] : SE_PARTS, s);
        }
        case EDGEDET_OP_MAXPOOL: {
            namespace r = rec::maxpool;
            PoolParams p{};
            p.x = P<const float>(o, r::x);
            p.y = P<float>(o, r::y);
            p.B = (int)I[r::B];
            p.H = (int)I[r::H];
            p.W = (int)I[r::W];
            p.C = (int)I[r::C];
            p.Ho = (int)I[r::Ho];
            p.Wo = (int)I[r::Wo];
            p.K = (int)I[r::K];
            p.stride = (int)I[r::stride];
            p.pad = (int)I[r::pad];
            return maxpool_launch(p, s);
        }
        case EDGEDET_OP_SSD_SCORES: {
            namespace r = rec::ssd_scores;
            return ssd_scores_launch(P<const float>(o, r::logits), P<const float>(o, r::reg),
                                     P<const float>(o, r::anchors), P<float>(o, r::scores_t), P<float>(o, r::boxes),
                                     (int)I[r::B], (int)I[r::A], (int)I[r::NC], o.f[r::img_h], o.f[r::img_w], s);
        }
        case EDGEDET_OP_SSD_CLASS_NMS: {
            namespace r = rec::ssd_class_nms;
            return ssd_class_nms_launch(P<const float>(o, r::scores_t), P<const float>(o, r::boxes), (int)I[r::B],
                                        (int)I[r::A], (int)I[r::NC], o.f[r::score_thresh], (int)I[r::topk],
                                        o.d[r::iou], seg_out(o, r::records0, (int)I[r::kmax]), s);
        }
        case EDGEDET_OP_MERGE_TOPK: {
            namespace r = rec::merge_topk;
            MergeParams p{};
            p.box = P<const f32x4>(o, r::records0 + rec::seg::box);
            p.score = P<const float>(o, r::records0 + rec::seg::score);
            p.tb = P<const uint32_t>(o, r::records0 + rec::seg::tb);
            p.label = P<const int>(o, r::records0 + rec::seg::label);
            p.count = P<const int>(o, r::records0 + rec::seg::count);
            p.ratio = P<const float>(o, r::ratio);
            p.out_box = P<float>(o, r::out_box);
            p.out_score = P<float>(o, r::out_score);
            p.out_label = P<int64_t>(o, r::out_label);
            p.out_count = P<int>(o, r::out_count);
            p.S = (int)I[r::S];
            p.kmax = (int)I[r::kmax];
            p.N = (int)I[r::N];
            return merge_topk_launch(p, (int)I[r::B], s);
        }
        case EDGEDET_OP_RPN_LEVEL_NMS: {
            namespace r = rec::rpn_level_nms;
            RpnParams p{};
            p.B = (int)I[r::B];
            p.nlevels = (int)I[r::nlevels];
            p.ld = (int)I[r::ld];
            p.A = (int)I[r::A];
            p.topk = (int)I[r::topk];
            EDGEDET_REQUIRE(p.nlevels >= 1 && p.nlevels <= 5, "rpn: 1..5 levels");
            for (int l = 0; l < p.nlevels; ++l) {
                p.lv[l].obj = P<const float>(o, r::obj0 + l);
                p.lv[l].deltas = P<const float>(o, r::deltas0 + l);
                p.lv[l].anchors = P<const float>(o, r::anchors0 + l);
                p.lv[l].n = (int)I[r::n0 + l];
            }
            p.img_h = o.f[r::img_h];
            p.img_w = o.f[r::img_w];
            p.min_size = o.f[r::min_size];
            p.score_thresh = o.f[r::score_thresh];
            p.iou = make_iou_thr(o.d[r::iou]);
            p.ckey = P<uint32_t>(o, r::ckey);  // chunked top-k scratch (or null)
            p.cidx = P<int>(o, r::cidx);
            p.ccount = P<int>(o, r::ccount);
            p.chunk = (int)I[r::chunk];
            p.nchunk = (int)I[r::nchunk];
            p.split = P<void>(o, r::split);
            return rpn_level_nms_launch(p, seg_out(o, r::records0, (int)I[r::kmax]), s);
        }
        case EDGEDET_OP_ROI_ALIGN: {
            namespace r = rec::roi_align;
            RoiParams p{};
            for (int l = 0; l < 4; ++l) {
                p.feat[l] = P<const float>(o, r::feat0 + l);
                p.H[l] = (int)I[r::H0 + l];
                p.W[l] = (int)I[r::W0 + l];
                p.scale[l] = o.f[r::scale0 + l];
            }
            p.rois = P<const float>(o, r::rois);
            p.counts = P<const int>(o, r::counts);
            p.out = P<float>(o, r::out);
            p.mode = (int)I[r::mode];
            p.R = (int)I[r::R];
            p.RMAX = (int)I[r::RMAX];
            p.B = (int)I[r::B];
            p.C = (int)I[r::C];
            p.PH = (int)I[r::PH];
            p.PW = (int)I[r::PW];
            p.sr = (int)I[r::sr];
            p.nlevels = (int)I[r::nlevels];
            p.k_min = (int)I[r::k_min];
            p.k_max = (int)I[r::k_max];
            return roi_align_launch(p, s);
        }
        case EDGEDET_OP_BOX_SCORES: {
            namespace r = rec::box_scores;
            return box_scores_launch(P<const float>(o, r::pred), (int)I[r::ld], (int)I[r::cls_off],
                                     (int)I[r::delta_off], P<const float>(o, r::props), P<const int>(o, r::counts),
                                     P<float>(o, r::scores), P<float>(o, r::boxes), (int)I[r::B], (int)I[r::R],
                                     (int)I[r::NC], o.f[r::img_h], o.f[r::img_w], s);
        }
        case EDGEDET_OP_BOX_CLASS_NMS: {
            namespace r = rec::box_class_nms;
            return box_class_nms_launch(P<const float>(o, r::scores), P<const float>(o, r::boxes),
                                        P<const int>(o, r::counts), (int)I[r::B], (int)I[r::R], (int)I[r::NC],
                                        o.f[r::score_thresh], o.f[r::min_size], o.d[r::iou],
                                        seg_out(o, r::records0, (int)I[r::kmax]), s);
        }
        case EDGEDET_OP_GN_STATS: {
            namespace r = rec::gn_stats;
            GnParams p{};
            p.x = P<const float>(o, r::x);
            p.gamma = P<const float>(o, r::gamma);
            p.beta = P<const float>(o, r::beta);
            p.scale = P<float>(o, r::scale);
            p.shift = P<float>(o, r::shift);
            p.B = (int)I[r::B];
            p.HW = (int)I[r::HW];
            p.C = (int)I[r::C];
            p.G = (int)I[r::G];
            p.eps = o.f[r::eps];
            return gn_stats_launch(p, s);
        }
        case EDGEDET_OP_RETINA_SELECT: {
            namespace r = rec::retina_select;
            RetinaSelParams p{};
            p.logits = P<const float>(o, r::logits);
            p.deltas = P<const float>(o, r::deltas);
            p.anchors = P<const float>(o, r::anchors);
            p.B = (int)I[r::B];
            p.L = (int)I[r::L];
            p.Atot = (int)I[r::Atot];
            p.K = (int)I[r::K];
            p.topk = (int)I[r::topk];
            EDGEDET_REQUIRE(p.L >= 1 && p.L <= 5, "retina_select: 1..5 levels");
            for (int l = 0; l < p.L; ++l) {
                p.a0[l] = (int)I[r::first0 + l];
                p.na[l] = (int)I[r::count0 + l];
            }
            p.img_h = o.f[r::img_h];
            p.img_w = o.f[r::img_w];
            p.score_thresh = o.f[r::score_thresh];
            p.ckey = P<uint32_t>(o, r::ckey);
            p.cidx = P<int>(o, r::cidx);
            p.ccount = P<int>(o, r::ccount);
            p.chunk = (int)I[r::chunk];
            p.nchunk = (int)I[r::nchunk];
            return retina_select_launch(p, seg_out(o, r::records0, (int)I[r::kmax]), s);
        }
        case EDGEDET_OP_SSD_STEM: {
            namespace r = rec::ssd_stem;
            StemParams p{};
            p.x = P<const float>(o, r::x);
            p.w0 = P<const float>(o, r::w0);
            p.b0 = P<const float>(o, r::b0);
            p.wd = P<const float>(o, r::wd);
            p.bd = P<const float>(o, r::bd);
            p.w1 = P<const float>(o, r::w1);
            p.b1 = P<const float>(o, r::b1);
            p.y = P<float>(o, r::y);
            p.B = (int)I[r::B];
            p.H = (int)I[r::H];
            p.W = (int)I[r::W];
            p.Ho = (int)I[r::Ho];
            p.Wo = (int)I[r::Wo];
            p.ld0 = (int)I[r::ld0];
            p.ld1 = (int)I[r::ld1];
            p.src = P<const float>(o, r::src);  // the transform folded in: source image, its size and normalisation
            p.src8 = P<const uint8_t>(o, r::src8);
            p.H0 = (int)I[r::H0];
            p.W0 = (int)I[r::W0];
            for (int c = 0; c < 3; ++c) {
                p.mean[c] = o.f[r::mean0 + c];
                p.stdv[c] = o.f[r::std0 + c];
            }
            return ssd_stem_launch(p, s);
        }
        case EDGEDET_OP_RETINA_CLASS_NMS: {
            namespace r = rec::retina_class_nms;
            RetinaNmsParams p{};
            p.box = P<const f32x4>(o, r::level0 + rec::seg::box);
            p.score = P<const float>(o, r::level0 + rec::seg::score);
            p.label = P<const int>(o, r::level0 + rec::seg::label);
            p.count = P<const int>(o, r::level0 + rec::seg::count);
            p.L = (int)I[r::L];
            p.kin = (int)I[r::kin];
            p.K = (int)I[r::K];
            p.iou = make_iou_thr(o.d[r::iou]);
            return retina_class_nms_launch(p, (int)I[r::B], seg_out(o, r::records0, (int)I[r::kmax]), s);
        }
        case EDGEDET_OP_SSD_POSTPROCESS: {
            namespace r = rec::ssd_postprocess;
            SsdPostParams p{};
            p.scores_t = P<const float>(o, r::scores_t);
            p.boxes = P<const float>(o, r::boxes);
            p.pool_key = P<uint32_t>(o, r::pool_key);
            p.pool_ref = P<int>(o, r::pool_ref);
            p.ratio = P<const float>(o, r::ratio);
            p.out_box = P<float>(o, r::out_box);
            p.out_score = P<float>(o, r::out_score);
            p.out_label = P<int64_t>(o, r::out_label);
            p.out_count = P<int>(o, r::out_count);
            p.B = (int)I[r::B];
            p.A = (int)I[r::A];
            p.NC = (int)I[r::NC];
            p.topk = (int)I[r::topk];
            p.N = (int)I[r::N];
            p.select_wave = (int)I[r::select_wave];
            p.score_thresh = o.f[r::score_thresh];
            p.iou = o.d[r::iou];
            return ssd_postprocess_launch(p, s);
        }
        default:
            set_error("edgedet: unknown op kind " + std::to_string(o.kind));
            return -1;
    }
}

// Side streams and fork/join/wait events, one set per (device, caller stream), shared by every
// thread (cgo and other foreign hosts call from arbitrary OS threads): two plans in flight on two
// caller streams (run_batches) get disjoint side lanes, so their lane work overlaps instead of
// queueing on one shared side stream.  At most LANE_CACHE sets exist: a new caller stream beyond that
// takes over the least recently used set (re-keyed, never destroyed: the HIP runtime's captured graphs
// keep references to the streams and events they were captured with, and destroying them measured
// a segfault in a later hipGraphLaunch).  A set's mutex serialises issue into it, so two threads whose
// caller streams share a set still record and wait its events in a consistent order.
struct Lanes {
    hipStream_t side[EDGEDET_MAX_LANES] = {};
    hipEvent_t fork_ev = nullptr;
    hipEvent_t join_ev[EDGEDET_MAX_LANES] = {};
    std::vector<hipEvent_t> wait_ev;
    uint64_t last_use = 0;
    std::mutex mu;
    bool ensure_wait_events(size_t n) {
        while (wait_ev.size() < n) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
            wait_ev.push_back(e);
        }
        return true;
    }
};
constexpr size_t LANE_CACHE = 16;
static std::mutex g_lanes_mu;
static std::map<std::pair<int, hipStream_t>, Lanes*> g_lanes_by_stream;  // sets live for the process
static uint64_t g_lanes_clock = 0;

static Lanes* make_lanes() {
    auto* L = new Lanes();
    for (int l = 1; l < EDGEDET_MAX_LANES; ++l) {
        if (hipStreamCreateWithFlags(&L->side[l], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&L->join_ev[l], hipEventDisableTiming) != hipSuccess)
            return nullptr;  // (a partial set is leaked: creation failing means the device is unusable)
    }
    if (hipEventCreateWithFlags(&L->fork_ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    return L;
}

static Lanes* lanes_for(hipStream_t caller) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const auto key = std::make_pair(dev, caller);
    std::lock_guard<std::mutex> lock(g_lanes_mu);
    auto it = g_lanes_by_stream.find(key);
    if (it != g_lanes_by_stream.end()) {
        it->second->last_use = ++g_lanes_clock;
        return it->second;
    }
    Lanes* L = nullptr;
    size_t on_dev = 0;
    for (auto& kv : g_lanes_by_stream) on_dev += kv.first.first == dev;
    if (on_dev >= LANE_CACHE) {  // take over the least recently used set of this device
        auto lru = g_lanes_by_stream.end();
        for (auto i = g_lanes_by_stream.begin(); i != g_lanes_by_stream.end(); ++i)
            if (i->first.first == dev && (lru == g_lanes_by_stream.end() || i->second->last_use < lru->second->last_use))
                lru = i;
        L = lru->second;
        g_lanes_by_stream.erase(lru);
    } else {
        L = make_lanes();
        if (!L) return nullptr;
    }
    L->last_use = ++g_lanes_clock;
    g_lanes_by_stream[key] = L;
    return L;
}

static size_t lane_cache_size() {
    std::lock_guard<std::mutex> lock(g_lanes_mu);
    return g_lanes_by_stream.size();
}

// Lane topology of a record sequence, checked before anything is issued (so a refused plan leaves
// the streams, and a capture, untouched): every op runs on lane 0 or a forked side lane; FORK opens
// 1..3 side lanes from lane 0 (none open), JOIN closes them into lane 0; WAIT (lane i0 waits for
// everything issued so far on lane i1) connects two distinct open lanes.  Returns the WAIT count.
static int64_t check_topology(const edgedet_op* ops, int64_t n) {
    int forked = 0;
    int64_t waits = 0;
    for (int64_t k = 0; k < n; ++k) {
        const edgedet_op& o = ops[k];
        const std::string at = "op " + std::to_string(k) + ": ";
        if (o.kind == EDGEDET_OP_FORK) {
            EDGEDET_REQUIRE(forked == 0, at + "fork while side lanes are open");
            const int64_t lanes = o.i[rec::fork::lanes];
            EDGEDET_REQUIRE(lanes >= 1 && lanes < EDGEDET_MAX_LANES, at + "fork: 1..3 side lanes");
            forked = (int)lanes;
        } else if (o.kind == EDGEDET_OP_JOIN) {
            const int64_t lanes = o.i[rec::join::lanes];
            EDGEDET_REQUIRE(lanes >= 1 && lanes < EDGEDET_MAX_LANES && lanes == forked,
                            at + "join: the forked side lanes");
            forked = 0;
        } else if (o.kind == EDGEDET_OP_WAIT) {
            const int64_t a = o.i[rec::wait::waiter], b = o.i[rec::wait::waited];
            EDGEDET_REQUIRE(a >= 0 && b >= 0 && a != b && a <= forked && b <= forked,
                            at + "wait: two distinct forked lanes");
            ++waits;
        } else if (o.kind == EDGEDET_OP_GROUP) {
            // the next `members` records: all CONV or all DWCONV, on the GROUP record's lane
            const int64_t g = o.i[rec::group::members], lane = o.i[EDGEDET_OP_LANE];
            EDGEDET_REQUIRE(g >= 1 && g <= EDGEDET_MAX_GROUP && k + g < n, at + "group: 1..12 following records");
            EDGEDET_REQUIRE(lane >= 0 && lane < EDGEDET_MAX_LANES && (lane == 0 || lane <= forked),
                            at + "group on a lane that is not forked");
            const int64_t kind = ops[k + 1].kind;
            EDGEDET_REQUIRE(kind == EDGEDET_OP_CONV || kind == EDGEDET_OP_DWCONV, at + "group: CONV or DWCONV members");
            for (int64_t j = k + 1; j <= k + g; ++j) {
                EDGEDET_REQUIRE(ops[j].kind == kind && ops[j].i[EDGEDET_OP_LANE] == lane,
                                at + "group: members of one kind on the group's lane");
                // one grouped launch runs one tile: run_group resolves member 0's requested tile
                // for every member, so members requesting different tiles are refused here
                EDGEDET_REQUIRE(kind != EDGEDET_OP_CONV || ops[j].i[rec::conv::tile] == ops[k + 1].i[rec::conv::tile],
                                at + "group: CONV members requesting different tiles (i23)");
            }
            k += g;
        } else {
            const int64_t lane = o.i[EDGEDET_OP_LANE];
            EDGEDET_REQUIRE(lane >= 0 && lane < EDGEDET_MAX_LANES && (lane == 0 || lane <= forked),
                            at + "op on a lane that is not forked");
        }
    }
    EDGEDET_REQUIRE(forked == 0, "plan ends with side lanes still forked (missing JOIN)");
    return waits;
}

// A GROUP's members as one grouped launch (conv_group_launch / dwconv_group_launch); members that
// cannot share a kernel variant are issued one by one (same results, more launches).
static int run_group(const edgedet_op* m, int n, hipStream_t s) {
    int rc = 1;
    if (diag_skip_mask() >> (m[0].kind & 63) & 1) return 0;
    if (m[0].kind == EDGEDET_OP_CONV) {
        ConvParams ps[EDGEDET_MAX_GROUP];
        for (int k = 0; k < n; ++k) {
            ps[k] = conv_params(m[k]);
            EDGEDET_REQUIRE(ps[k].K == ps[k].KH * ps[k].KW * ps[k].Cin, "conv: K != KH*KW*Cin");
        }
        rc = conv_group_launch(ps, n, (int)m[0].i[rec::conv::tile], s);
    } else {
        DwParams ps[EDGEDET_MAX_GROUP];
        for (int k = 0; k < n; ++k) ps[k] = dw_params(m[k]);
        rc = dwconv_group_launch(ps, n, s);
    }
    if (rc <= 0) return rc;
    for (int k = 0; k < n; ++k) {
        const int r = run_op(m[k], s);
        if (r) return r;
    }
    return 0;
}

static int run_ops(const edgedet_op* ops, int64_t n, hipStream_t s) {
    const int64_t waits = check_topology(ops, n);
    if (waits < 0) return (int)waits;
    bool need_lanes = false;
    for (int64_t k = 0; k < n && !need_lanes; ++k)
        need_lanes = ops[k].kind == EDGEDET_OP_FORK || ops[k].i[EDGEDET_OP_LANE] != 0;
    Lanes* lanes = need_lanes ? lanes_for(s) : nullptr;
    EDGEDET_REQUIRE(!need_lanes || lanes, "could not create the side lanes (streams / events)");
    std::unique_lock<std::mutex> issue;
    if (lanes) issue = std::unique_lock<std::mutex>(lanes->mu);
    EDGEDET_REQUIRE(!waits || lanes->ensure_wait_events((size_t)waits), "could not create the wait events");
    auto lane_stream = [&](int64_t l) { return l == 0 ? s : lanes->side[l]; };
    int64_t wait_k = 0;
    for (int64_t k = 0; k < n; ++k) {
        const edgedet_op& o = ops[k];
        int rc = 0;
        if (o.kind == EDGEDET_OP_FORK) {
            EDGEDET_CHECK_HIP(hipEventRecord(lanes->fork_ev, s));
            for (int l = 1; l <= (int)o.i[rec::fork::lanes]; ++l)
                EDGEDET_CHECK_HIP(hipStreamWaitEvent(lanes->side[l], lanes->fork_ev, 0));
        } else if (o.kind == EDGEDET_OP_JOIN) {
            for (int l = 1; l <= (int)o.i[rec::join::lanes]; ++l) {
                EDGEDET_CHECK_HIP(hipEventRecord(lanes->join_ev[l], lanes->side[l]));
                EDGEDET_CHECK_HIP(hipStreamWaitEvent(s, lanes->join_ev[l], 0));
            }
        } else if (o.kind == EDGEDET_OP_WAIT) {
            hipEvent_t e = lanes->wait_ev[(size_t)wait_k++];
            EDGEDET_CHECK_HIP(hipEventRecord(e, lane_stream(o.i[rec::wait::waited])));
            EDGEDET_CHECK_HIP(hipStreamWaitEvent(lane_stream(o.i[rec::wait::waiter]), e, 0));
        } else if (o.kind == EDGEDET_OP_GROUP) {
            const int64_t g = o.i[rec::group::members];
            rc = run_group(ops + k + 1, (int)g, lane_stream(o.i[EDGEDET_OP_LANE]));
            k += g;
        } else {
            rc = run_op(o, lane_stream(o.i[EDGEDET_OP_LANE]));
        }
        if (rc != 0) {
            set_error("op " + std::to_string(k) + " (kind " + std::to_string(o.kind) + "): " + g_error);
            return rc;
        }
    }
    return 0;
}

struct Graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};
// Live graphs: launch and destroy refuse a handle that is not one (a destroyed or foreign pointer
// would otherwise reach hipGraphLaunch and crash the host process).
static std::mutex g_graphs_mu;
static std::set<Graph*> g_graphs;

}  // namespace edgedet

using namespace edgedet;

extern "C" int edgedet_plan_run(const edgedet_op* ops, int64_t n, void* stream) {
    return run_ops(ops, n, (hipStream_t)stream);
}

extern "C" int edgedet_plan_check(const edgedet_op* ops, int64_t n) {
    const int64_t w = check_topology(ops, n);
    return w < 0 ? (int)w : 0;
}

extern "C" int edgedet_release_lanes(void* stream) {
    int dev = 0;
    EDGEDET_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_lanes_mu);
    auto it = g_lanes_by_stream.find(std::make_pair(dev, (hipStream_t)stream));
    if (it != g_lanes_by_stream.end()) it->second->last_use = 0;  // first to be taken over
    return 0;
}

extern "C" int64_t edgedet_lane_sets(void) { return (int64_t)lane_cache_size(); }

extern "C" int edgedet_graph_create(const edgedet_op* ops, int64_t n, void* stream, void** out) {
    hipStream_t s = (hipStream_t)stream;
    EDGEDET_REQUIRE(s != nullptr, "graph capture needs a non-default stream");
    {  // refuse a bad topology before the capture begins
        const int64_t w = check_topology(ops, n);
        if (w < 0) return (int)w;
    }
    Graph* g = new Graph();
    {
        const hipError_t eb = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
        if (eb != hipSuccess) {
            delete g;
            set_error(std::string("hipStreamBeginCapture: ") + hipGetErrorString(eb));
            return -2;
        }
    }
    const int rc = run_ops(ops, n, s);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != 0) {
        if (graph) (void)hipGraphDestroy(graph);
        delete g;
        return rc;
    }
    if (e != hipSuccess) {
        delete g;
        set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        return -2;
    }
    g->graph = graph;
    const hipError_t e2 = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
        (void)hipGraphDestroy(graph);
        delete g;
        set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e2));
        return -2;
    }
    // upload the executable graph now (its kernel-node packets and argument buffers onto the device),
    // so the first hipGraphLaunch does not pay for it inside a caller's timed or served batch
    const hipError_t eu = hipGraphUpload(g->exec, s);
    if (eu != hipSuccess) {
        (void)hipGraphExecDestroy(g->exec);
        (void)hipGraphDestroy(graph);
        delete g;
        set_error(std::string("hipGraphUpload: ") + hipGetErrorString(eu));
        return -2;
    }
    {
        std::lock_guard<std::mutex> lock(g_graphs_mu);
        g_graphs.insert(g);
    }
    *out = g;
    return 0;
}

extern "C" int edgedet_graph_launch(void* graph, void* stream) {
    Graph* g = reinterpret_cast<Graph*>(graph);
    {
        std::lock_guard<std::mutex> lock(g_graphs_mu);
        EDGEDET_REQUIRE(g && g_graphs.count(g) && g->exec, "graph_launch: not a live graph (null or destroyed)");
    }
    EDGEDET_CHECK_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return 0;
}

extern "C" int edgedet_graph_destroy(void* graph) {
    Graph* g = reinterpret_cast<Graph*>(graph);
    if (!g) return 0;
    {
        std::lock_guard<std::mutex> lock(g_graphs_mu);
        EDGEDET_REQUIRE(g_graphs.erase(g) == 1, "graph_destroy: not a live graph (destroyed twice?)");
    }
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return 0;
}

// The conv kernel variant (tile id, csrc/conv.hip conv_launch) a CONV record runs, without launching.
extern "C" int edgedet_conv_tile(const edgedet_op* op) {
    EDGEDET_REQUIRE(op && op->kind == EDGEDET_OP_CONV, "conv_tile: not a CONV record");
    ConvParams p = conv_params(*op);
    const int rc = conv_prepare(p);
    if (rc) return rc;
    return conv_resolve_tile(p, (int)op->i[rec::conv::tile]);
}

extern "C" const char* edgedet_last_error(void) { return get_error(); }
extern "C" int32_t edgedet_version(void) { return (1 << 16) | 0; }
extern "C" const char* edgedet_target(void) { return "gfx950"; }
