// yn_api.hip — the C ABI of libyolonano_hip.so (see include/yolonano_hip.h) and the network executor.
//
// The handle owns: the raw parameters (reference state-dict keys), the folded + packed weights, one
// activation arena in HBM, NMS scratch, and optional hipGraphs of the fixed-shape pipelines.
// Network wiring restates models/yolo_nano.py:282-301 and backbone/shufflenetv2.py:69-78,157-167.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/yolonano_hip.h"
#include "yn_internal.h"
#include "yn_h16.h"
#include <stdlib.h>

using namespace ynk;

namespace {

thread_local std::string g_create_error;
std::mutex g_tune_mutex;
std::map<std::vector<int>, int> g_pw_tuned;        // (device, M, K, N, strides...) -> fastest pointwise tile configuration

struct Param {
    DevBuf<float> dev;                     // [numel]
    size_t numel = 0;
    std::vector<int64_t> shape;
};

enum { K_PW = 0, K_DW = 1, K_DENSE3 = 2, K_STEM = 3 };

struct Layer {
    std::string name, conv, bn;
    int kind = 0, cin = 0, cout = 0, stride = 1, has_bias = 0, act = 0;
    DevBuf<float> w_packed, b_packed, w_ref, b_ref;
    DevBuf<_Float16> ws_hi, ws_lo;         // split-f16 packs of the folded weights (dense 3x3: conv3x3_split_kernel), equal sizes
    size_t ws_bytes() const { return ws_hi.cap() * sizeof(_Float16); }
    size_t w_numel = 0;
    int Kp = 0, Npad = 0;
};

struct TrainPack { DevBuf<float> wp, bias, wp_bwd; int Kb = 0, Npad_b = 0; };   // per-layer training weight packs

// per-layer weight packs of the fp16 training step (yn_train_h16.inc): f16 GEMM packs (forward / input gradient), fp32 depthwise taps
struct HPack { DevBuf<ynk::h16> wf, wb; DevBuf<float> bias, dwf, dwb; int Kp = 0, Npad = 0, Kpb = 0, Npadb = 0; };

struct ProfRec {
    std::string name, kernel;
    hipEvent_t e0, e1;
    double flops, bytes;
};

struct TrainGraph { std::vector<uintptr_t> key; hipGraphExec_t exec; int direct_runs; };      // the fp16 training step's body as a graph (yn_train_h16.inc)
struct GraphEntry {
    std::vector<uintptr_t> key;
    hipGraphExec_t exec = nullptr;
};

}  // namespace

struct yn_coco { ynk::CocoState* st; };      // likewise (kernels_coco.hip)
struct yn_kmeans { ynk::KmeansState* st; };  // likewise (kernels_kmeans.hip)
struct yn_draw { ynk::DrawState* st; };      // likewise (kernels_draw.hip)
struct yn_track { ynk::TrackState* st; };    // likewise (kernels_track.hip)
struct yn_chip { ynk::ChipState* st; };      // likewise (kernels_chip.hip)
struct yn_jpeg { ynk::JpegState* st; };      // likewise (kernels_jpeg.hip)
struct yn_jpeg_enc { ynk::JpegEncState* st; };      // likewise (kernels_jpeg_enc.hip)
struct yn_eval { ynk::EvalState* st; };      // opaque to callers: its own lifetime, launches on the stream of the handle passed per call
namespace {

// DevBuf::reserve for the members of an object that is allocated in one go: after the first failure nothing more is tried
struct Reserve {
    int rc = 0;                                                      // the first failure's code (a hipError_t), 0: none
    size_t failed = 0;                                               // its bytes
    template <class Buf> void operator()(Buf& buf, size_t n) { if (!rc && (rc = buf.reserve(n)) != 0) failed = n * sizeof(buf[0]); }
};

// yn_infer's outputs for one forward of yn_tta / yn_slice
struct InferOut {
    ynk::DevBuf<float> fb, fs; ynk::DevBuf<int32_t> fc, fcount;      // [images][N] ([4] per box), [images]
    void reserve(Reserve& take, size_t images, size_t N) { take(fb, images * N * 4); take(fs, images * N); take(fc, images * N); take(fcount, images); }
};

// What yn_tta and yn_slice end in ("The merge lists and the merge"): one merge list per unit (an image / a frame) that the object's append kernel fills, ONE read-back of
// the state words (MERGE_STATE, yn_internal.h), per-class NMS, yn_pack_detections into rec / offsets.  Allocated once, for `units` lists of `cap` rows.
struct MergeLists {
    int device = 0, cap = 0, A = 0, C = 0, units = 0;                // units: the object's max_batch / max_frames
    ynk::DevBuf<float> lb, ls; ynk::DevBuf<int32_t> lc;              // the merge lists [units][cap]
    ynk::DevBuf<int32_t> state;                                      // [MERGE_STATE + units]: flags + cursors (the append kernels)
    ynk::DevBuf<float> mb, ms; ynk::DevBuf<int32_t> mc, mcount;      // the merge's kept rows [units][cap]
    ynk::DevBuf<float> rec; ynk::DevBuf<int32_t> offsets;            // yn_pack_detections layout: [units * cap][6], [units + 1]
    std::vector<int32_t> state_host;                                 // the one read-back of merge()
    int lists_n = -1;                                                // units whose merge lists are valid (copy_lists), -1: none
    int last_n = -1;                                                 // units of the last successful merge() / empty_result(), -1: none
    int total = -1;                                                  // offsets[last_n], read on the first result() that asks for it
    hipStream_t last_stream = nullptr;

    void reserve(Reserve& take, const yn_config& cfg, int units, int cap);
    bool clear_once(hipStream_t s);
    int belongs(yn_handle* h, const char* who) const;
    void drop_result() { last_n = -1; total = -1; }
    int open(yn_handle* h, int n);
    int rule = YN_MERGE_NMS, expected = 0;                           // the merge rule (yn_*_merge_rule); expected 0: the client's default
    int set_rule(yn_handle* h, const char* who, int rule_, int expected_);
    int soft = YN_SOFT_OFF; float soft_sigma = 0.5f, soft_floor = 0.0f;      // how the YN_MERGE_NMS rule suppresses (yn_merge_soft_*)
    int set_soft(yn_handle* h, const char* who, int method, float sigma, float score_floor);
    int merge(yn_handle* h, const char* who, const char* unit, int n, float thresh, int default_expected);
    int empty_result(yn_handle* h, int n);
    int result(const float** rec_dev, const int32_t** offsets_dev, int32_t* total_out);
    int copy_lists(yn_handle* h, int n, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host) const;
};

}  // namespace

// test-time augmentation for whole batches (kernels_tta.hip): every buffer is allocated once, for max_batch images and the largest scale
struct yn_tta {
    int flip = 1, max_batch = 0, Nmax = 0, smax = 0;
    std::vector<int> scales;
    ynk::DevBuf<float> xr;                                           // the resized (+ mirrored) batch [nb][3][smax][smax], nb = flip ? 2 max_batch : max_batch
    InferOut f;                                                      // yn_infer's outputs for one scale: [nb][Nmax]
    ynk::DevBuf<int32_t> fstart;                                     // [forwards][max_batch]
    MergeLists m;                                                    // one list per image
};

// sliced inference (kernels_slice.hip): the merge lists and the result are allocated once, for max_frames frames; the tile batch and yn_infer's
// outputs of one chunk follow the handle's grid and max_batch on the first yn_slice_infer that needs them
struct yn_slice {
    ynk::DevBuf<float> x;                                            // one chunk of tiles [max_batch][3][side][side] (yn_slice_infer)
    InferOut f;                                                      // yn_infer's outputs for it: [max_batch][N]
    ynk::DevBuf<int32_t> tstart;                                     // [T] of the current table
    MergeLists m;                                                    // one list per frame; lists_n = the frames of the table being appended
    int lists_T = 0, next_t = 0;                                     // that table's tiles, the tile the next chunk starts at
};

// record lists fused per unit (kernels_wbf.hip): the third client of the merge lists
struct yn_fuse {
    MergeLists m;                                                    // one list per unit
    int appends = 0;                                                 // yn_fuse_append calls since yn_fuse_open: the default `expected`
};

struct yn_handle {
    yn_config cfg;
    hipStream_t stream = nullptr;
    hipStream_t cur = nullptr;            // stream the launch helpers currently target (main or a side stream)
    hipStream_t side[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> fj_events;    // fork/join events (rotating pool)
    size_t fj_next = 0;
    bool multi_stream = true;
    std::string err;
    std::map<std::string, Param> params;
    std::vector<Layer> layers;
    std::map<std::string, int> by_name;
    std::map<std::string, int> by_conv;
    bool folded = false;
    int stage_ch[3] = {0, 0, 0};
    int head_ch = 0;
    GridInfo grid;
    // arena
    DevBuf<char> arena;                   // the activations, then the sync words of stage_pipe_kernel
    size_t arena_bytes = 0, arena_used = 0;       // bytes of the activation part / taken from it
    int arena_S = 0, arena_B = 0;
    // candidate buffers + NMS scratch (ensure_post): per candidate [B*N], per segment [B*(C+1)], the suppression matrix, the prefilter's slice sync
    DevBuf<float> cand_boxes, cand_scores, nms_sbox, nms_sbox2;
    DevBuf<int32_t> cand_cls, nms_bucket, nms_keep, nms_bucket2;
    DevBuf<int32_t> nms_seg[10];          // seg_count, seg_off, tile_off, large_list, seg_count2, tile_off2, seg_order, seg_sparse, work_off, ctr
    DevBuf<unsigned long long> nms_matrix, nms_pre_sync;
    NmsWork nms{};                        // the view of that scratch launch_nms_pipeline takes, filled by ensure_post
    DevBuf<float> wbf_box, wbf_score, wbf_ofb, wbf_op, wbf_os;       // weighted box fusion's side and overflow arrays (ensure_wbf), [B*N] each ([4] per box)
    DevBuf<int32_t> wbf_votes, wbf_index, wbf_on, wbf_ofounder;
    WbfWork wbf{};                        // the view of them launch_wbf_pipeline takes
    DevBuf<float> soft_score, soft_spill; // Soft-NMS's side scores and spilled scores (ensure_soft, allocated on the first soft call), [B*N] each
    SoftWork soft{};                      // the view of them launch_soft_pipeline takes
    int soft_method = YN_SOFT_OFF;        // how yn_infer's / yn_postprocess's NMS suppresses (yn_soft_nms)
    float soft_sigma = 0.5f, soft_floor = 0.0f;
    NmsPlan nms_plan{};                   // launch_nms_pipeline's decisions in the last yn_postprocess / yn_infer / yn_nms_merge (yn_nms_stages; B = 0: none yet)
    DevBuf<float> heads_buf;              // the three raw head tensors, one block
    float* heads_int[3] = {nullptr, nullptr, nullptr};    // its split for the current grid (ensure_heads)
    float* fwd_only[3] = {nullptr, nullptr, nullptr};     // yn_train_forward: the training executors stop after the forward pass and copy the raw heads here
    float* tap_out[3] = {nullptr, nullptr, nullptr};      // yn_forward_taps: where run_network copies c3 / c4 / c5
    DevBuf<float> loss_partial;
    // training (yn_train.inc): caller-owned flat buffers + per-layer packs + workspace
    float *tP = nullptr, *tG = nullptr, *tM = nullptr;
    int64_t tN = 0, tN_expected = 0;
    long train_steps = 0;
    std::map<std::string, size_t> toff;
    std::vector<TrainPack> tpacks;
    DevBuf<float> zeros;
    DevBuf<float> train_losses;           // device float[4]: the step's body writes its losses here (a fixed address for the graph), copied to the caller's buffer afterwards
    std::vector<TrainGraph> train_graphs; int train_graph_misses = 0; bool train_graph = false; int64_t train_graph_replays = 0;   // yn_train_graph
    int head_fork = -1, head_fork_now = 0, fork_trials = 0;      // -1: undecided (steps 3-6 time the step with and without the forks), else the choice
    hipEvent_t fork_ev[8] = {};           // timing events of the trials
    hipStream_t train_fork[2] = {nullptr, nullptr};      // the head towers of levels 3 / 4 (forward and backward) beside the main stream
    hipStream_t train_side = nullptr;     // the fp16 step's weight-gradient stream (lowest priority: the main stream is the critical path)
    DevBuf<int> skip_flag;                // device int[2]: [0] this step's gradient is non-finite, [1] number of skipped updates
    int train_dtype = 0;                  // 0 fp32, 1 fp16 storage + f16 MFMA (yn_train_precision)
    std::vector<HPack> hpacks;
    std::vector<ynk::HPackDesc> hpack_jobs;   // recorded while the first fp16 step packs layer by layer; later steps pack everything in one launch
    DevBuf<ynk::HPackDesc> hpack_table;        // device copy
    DevBuf<float> scale_state;            // device float[8]: loss scale, its inverse, clean-step counter, local overflow flag, step-pending mark (kernels_h16.hip)
    float loss_scale_init = 0.0f, loss_scale_clean = 0.0f;   // yn_train_set_loss_scale before the first fp16 step (checkpoint resume)
    std::vector<hipEvent_t> train_events;
    DevBuf<char> train_arena;
    // graphs / profiling
    bool use_graph = false;
    bool tail_fuse = true;                 // yn_tail_fuse: off = layers .2+.3 and .4+decode of the heads as two grouped kernels instead of one (head_tail_group_kernel)
    bool down_fuse = true;                 // yn_down_fuse: the main branch of a stride-2 unit as one kernel (down_unit_pipe_kernel)
    bool group_launch = true;              // yn_group_launch: the three heads' layers (and the laterals) as grouped launches
    bool fuse_decode = true;               // yn_fuse_decode: yn_infer's last head conv + candidate decode as one kernel
    int fuse_decode_mode = 1;              // 1 = when the stride-8 head has >= 8192 pixels, 2 = always
    bool exact_f32 = false;                // yn_exact_f32: GEMM-shaped convs on the f32 MFMA only (no split-f16 operands)
    bool range_fallback = false;           // yn_fold_bn found a folded GEMM weight outside the split's range (|w| >= 65504): same effect as exact_f32
    PinnedBuf<unsigned, hipHostMallocMapped | hipHostMallocCoherent> range_host;   // one word of pinned host memory: set by compact_kernel beside the negative counts (the range flag, out of band);
    unsigned* range_host_dev = nullptr;    // its device view.  While set, yn_infer / yn_pack_detections return YN_STATUS_RANGE; yn_range_status clears it
    DevBuf<unsigned> range_flags;          // device uint[3]: [0] weights out of range (fold_pack_kernel), [1] an activation >= 65504 was split
                                           // (range_report, yn_device.h; read and cleared by yn_range_status), [2] the same as [0] for a yn_op_* call
    bool autotune = true;
    int force_pw_cfg = -1;                         // yn_set_pw_config (testing aid)
    int unit_chain = 1;                            // stride-1 ShuffleV2 units as one kernel each: 0 off, 1 where the map is large enough, 2 always (yn_unit_chain)
    bool pw_pipe = true;                           // pw_pipe_kernel among the pointwise candidates (yn_pw_pipe)
    int chain_pipe = 1;                            // unit_pipe_kernel (the persistent per-unit walk): 0 never, 1 by the size rule, 2 always (yn_chain_pipe)
    int stage_fuse = 1;                            // all but the last stride-1 unit of a stage as ONE persistent launch (stage_pipe_kernel): 0 off, 1 from 256 tiles, 2 always (yn_stage_fuse)
    int stage_pub_early = 0;                       // its tiles raise their ready flag right behind their stores (1) or under the next tile's depthwise phase (0, default: 608 x 608 stage 3 144 vs 150 us, 0.5x bs 128 101 vs 105, 416 bs 32 equal) (yn_stage_fuse publish_early)
    unsigned* stage_sync = nullptr;                // its queue heads / ready flags / exit count: behind the activation arena, zero between launches
    size_t stage_sync_bytes = 0;
    hipEvent_t tune_e0 = nullptr, tune_e1 = nullptr;
    std::vector<GraphEntry> graphs;
    bool profiling = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
};

namespace {

int fail(yn_handle* h, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return 1;
}

// Every entry point runs with the handle's device current and restores the caller's afterwards (a handle created on
// cuda:1 may be called while cuda:0 is current: its allocations, launches and hipFuncSetAttributes must not land there).
struct DevGuard : DeviceScope {
    explicit DevGuard(const yn_handle* h) : DeviceScope(h->cfg.device) {}
};
#define YN_ENTER(h) if (!(h)) return 1; DevGuard dev_guard_(h)

#define HIPCHK(h, expr)           /* a HIP call, or a DevBuf growth (its int is a hipError_t) */   \
    do {                                                                                           \
        hipError_t e_ = (hipError_t)(expr);                                                                 \
        if (e_ != hipSuccess) return fail((h), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// the f32-MFMA family runs every GEMM-shaped conv when the caller asked for it or when the folded weights do not fit the split
inline bool exact(const yn_handle* h) { return h->exact_f32 || h->range_fallback; }

const int STAGE_CH[4][3] = {{48, 96, 192}, {116, 232, 464}, {176, 352, 704}, {244, 488, 976}};
const int STAGE_REP[3] = {4, 8, 4};
const int NECK = 96;

void add_layer(yn_handle* h, const std::string& name, const std::string& conv, const std::string& bn,
               int kind, int cin, int cout, int stride, int has_bias, int act)
{
    Layer L;
    L.name = name; L.conv = conv; L.bn = bn; L.kind = kind; L.cin = cin; L.cout = cout;
    L.stride = stride; L.has_bias = has_bias; L.act = act;
    h->by_name[name] = (int)h->layers.size();
    h->by_conv[conv] = (int)h->layers.size();
    h->layers.push_back(std::move(L));
}

// the 77 convolutions, same naming as yolo_nano_amd/arch.py conv_specs()
void build_layers(yn_handle* h)
{
    char p[128], a[160], b[160];
    const int* sc = STAGE_CH[h->cfg.backbone];
    for (int i = 0; i < 3; ++i) h->stage_ch[i] = sc[i];
    add_layer(h, "stem", "backbone.conv1.0", "backbone.conv1.1", K_STEM, 3, 24, 2, 0, YN_ACT_RELU);
    int cin = 24;
    for (int si = 0; si < 3; ++si) {
        const int cout = sc[si], bf = cout / 2;
        for (int bi = 0; bi < STAGE_REP[si]; ++bi) {
            snprintf(p, sizeof p, "backbone.stage%d.%d", si + 2, bi);
            const std::string P = p;
            if (bi == 0) {
                add_layer(h, P + ".b1.dw", P + ".branch1.0", P + ".branch1.1", K_DW, cin, cin, 2, 0, YN_ACT_NONE);
                add_layer(h, P + ".b1.pw", P + ".branch1.2", P + ".branch1.3", K_PW, cin, bf, 1, 0, YN_ACT_RELU);
            }
            const int b2in = bi == 0 ? cin : bf;
            add_layer(h, P + ".b2.pw1", P + ".branch2.0", P + ".branch2.1", K_PW, b2in, bf, 1, 0, YN_ACT_RELU);
            add_layer(h, P + ".b2.dw", P + ".branch2.3", P + ".branch2.4", K_DW, bf, bf, bi == 0 ? 2 : 1, 0, YN_ACT_NONE);
            add_layer(h, P + ".b2.pw2", P + ".branch2.5", P + ".branch2.6", K_PW, bf, bf, 1, 0, YN_ACT_RELU);
        }
        cin = cout;
    }
    for (int i = 0; i < 3; ++i) {
        snprintf(a, sizeof a, "conv1x1_%d", i);
        add_layer(h, a, std::string(a) + ".convs.0", std::string(a) + ".convs.1", K_PW, sc[i], NECK, 1, 1, YN_ACT_LEAKY);
    }
    for (int i = 0; i < 4; ++i) {
        snprintf(a, sizeof a, "smooth_%d", i);
        add_layer(h, a, std::string(a) + ".convs.0", std::string(a) + ".convs.1", K_DENSE3, NECK, NECK, 1, 1, YN_ACT_LEAKY);
    }
    h->head_ch = h->cfg.num_anchors * (1 + h->cfg.num_classes + 4);
    for (int hd = 1; hd <= 3; ++hd) {
        for (int j = 0; j < 4; ++j) {
            snprintf(a, sizeof a, "head_det_%d.%d", hd, j);
            snprintf(b, sizeof b, "head_det_%d.%d.convs", hd, j);
            add_layer(h, a, std::string(b) + ".0", std::string(b) + ".1", (j & 1) ? K_PW : K_DW, NECK, NECK, 1, 1, YN_ACT_LEAKY);
        }
        snprintf(a, sizeof a, "head_det_%d.4", hd);
        add_layer(h, a, a, "", K_PW, NECK, h->head_ch, 1, 1, YN_ACT_NONE);
    }
}

// The grid of an H x W canvas that is the window at (left, top) of a letterboxed side x side square (include/yolonano_hip.h, yn_set_grid_rect);
// the window that is the whole square is the square grid (win = 0, S = side).  The caller has validated the window.
int set_grid_window(yn_handle* h, int H, int W, int side, int left, int top)
{
    GridInfo& g = h->grid;
    g.win = (H == W && W == side && left == 0 && top == 0) ? 0 : 1;
    g.S = g.win ? 0 : side; g.C = h->cfg.num_classes; g.A = h->cfg.num_anchors;
    g.H = H; g.W = W; g.side = side; g.left = left; g.top = top;
    int off = 0;
    for (int s = 0; s < 3; ++s) {
        const int w = W / (8 << s), hh = H / (8 << s);
        g.w[s] = w; g.h[s] = hh; g.hw[s] = hh * w; g.off[s] = off;
        off += hh * w * g.A;
    }
    g.N = off;
    g.head_ld = g.A * (5 + g.C);
    for (int i = 0; i < 18; ++i) g.anchors[i] = h->cfg.anchors[i];
    return 0;
}

int set_grid_info(yn_handle* h, int S)
{
    if (S <= 0 || (S % 32) != 0) return fail(h, "input_size %d is not a positive multiple of 32", S);
    return set_grid_window(h, S, S, S, 0, 0);
}

// the entries that stay square in this library (training, loss, targets, test-time augmentation): refused on a window grid, nothing launched
int need_square_grid(yn_handle* h, const char* who)
{
    if (!h->grid.win) return 0;
    return fail(h, "%s needs a square grid: the handle holds the %d x %d window at (%d, %d) of a %d square (yn_set_grid_rect)", who, h->grid.H, h->grid.W,
                h->grid.left, h->grid.top, h->grid.side);
}

const Param* find_param(yn_handle* h, const std::string& key)
{
    auto it = h->params.find(key);
    return it == h->params.end() ? nullptr : &it->second;
}

// ---- arena ------------------------------------------------------------------------------------
size_t network_arena_bytes(yn_handle* h, int B, int H, int W)
{
    // generous closed form: every buffer of run_network(), no reuse across stages (H and W are multiples of 32: every division is exact)
    const size_t px2 = (size_t)B * (H / 2) * (W / 2), px4 = px2 / 4;
    size_t fl = px2 * 24 + px4 * 24;
    int cin = 24;
    size_t cur = px4;
    for (int si = 0; si < 3; ++si) {
        const int C = h->stage_ch[si], bf = C / 2;
        const size_t po = cur / 4;
        fl += po * cin + po * bf + cur * bf + po * bf + 2 * po * C;
        cin = C; cur = po;
    }
    const size_t p3 = (size_t)B * (H / 8) * (W / 8), p4 = p3 / 4, p5 = p4 / 4;
    fl += (p3 + p4 + p5) * NECK * 2 + p4 * NECK;      // laterals, smoothed (p4 twice)
    fl += (p3 + p4 + p5) * NECK * 3;                   // head scratch, one set per (concurrent) head
    return fl * sizeof(float) + 192 * 256;           // (rounding + 16 bytes of slack per buffer: arena_take)
}
size_t network_arena_bytes(yn_handle* h, int B, int S) { return network_arena_bytes(h, B, S, S); }

// every cached hipGraphExec_t refers to the buffers it was captured with: destroy them whenever those go away
void drop_train_graphs(yn_handle* h)
{
    if (!h->train_graphs.empty()) (void)hipStreamSynchronize(h->stream);
    for (TrainGraph& g : h->train_graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->train_graphs.clear();
}

void drop_graphs(yn_handle* h)
{
    drop_train_graphs(h);
    if (!h->graphs.empty()) (void)hipStreamSynchronize(h->stream);     // a replay may still be in flight (the setters below reach here without draining)
    for (GraphEntry& g : h->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

int ensure_arena(yn_handle* h, int B, int H, int W)
{
    const size_t need = network_arena_bytes(h, B, H, W);
    if (need <= h->arena_bytes) return 0;
    if (h->arena) HIPCHK(h, hipStreamSynchronize(h->stream));
    // behind the activations: the sync words of stage_pipe_kernel (kernels_stage.hip) for the largest stage (stage 2: B (H/8)(W/8) rows, 32-row tiles,
    // up to YN_STAGE_MAX units).  Zeroed HERE, once, on the handle's stream; every launch leaves them zero.
    const size_t sync_bytes = (stage_sync_words((int)((size_t)B * (H / 8) * (W / 8) / 32 + 1), YN_STAGE_MAX) * sizeof(unsigned) + 255) & ~(size_t)255;
    h->arena_bytes = 0; h->stage_sync = nullptr; h->stage_sync_bytes = 0;
    bool moved = false;
    const int rc = h->arena.reserve(need + sync_bytes, 0, &moved);
    if (moved) drop_graphs(h);
    if (rc) return fail(h, "activation arena of %zu bytes: %s", need + sync_bytes, hipGetErrorString((hipError_t)rc));
    h->arena_bytes = need;
    h->stage_sync = reinterpret_cast<unsigned*>(h->arena + need);
    h->stage_sync_bytes = sync_bytes;
    HIPCHK(h, hipMemsetAsync(h->stage_sync, 0, sync_bytes, h->stream));
    return 0;
}

float* arena_take(yn_handle* h, size_t floats)
{
    // 16 bytes of slack behind every tensor: the LDS-DMA kernels fetch whole 16-byte pieces, and the last piece of a tensor's last row may run
    // up to 8 bytes past it (rows of 58 or 24 floats behind an 8-byte-aligned start) - never used, but it must be readable
    size_t bytes = (floats * sizeof(float) + 16 + 255) & ~(size_t)255;
    if (h->arena_used + bytes > h->arena_bytes) return nullptr;
    float* p = (float*)(h->arena + h->arena_used);
    h->arena_used += bytes;
    return p;
}

int ensure_post(yn_handle* h, int B, int N, int C)
{
    // worst case every candidate of an image falls into one class: that segment must fit resolve_segment()'s LDS mask
    if (N > nms_max_segment())
        return fail(h, "NMS over %d candidates per image exceeds the supported segment size %d", N, nms_max_segment());
    const size_t need = (size_t)B * N, need_seg = (size_t)B * (C + 1);
    const size_t m_stride = nms_matrix_words_per_image(N, C);
    const size_t need_ps = nms_pre_sync_words(B, N);
    // Every buffer answers for itself (a call that failed half way leaves each one empty or whole): the stream is drained before the first
    // block of a group goes, the graphs are dropped whenever an address changed, and the view is refilled on every way out.
    int rc = 0;
    bool moved = false, drained = false;
    auto take = [&](auto& buf, size_t n) {                  // true: buf is a new block
        if (rc || n <= buf.cap()) return false;
        if (!drained) { rc = (int)hipStreamSynchronize(h->stream); drained = true; }
        if (!rc) rc = buf.reserve(n, 0, &moved);
        return !rc;
    };
    take(h->cand_boxes, need * 4); take(h->cand_scores, need); take(h->cand_cls, need);
    take(h->nms_bucket, need); take(h->nms_keep, need); take(h->nms_sbox, need * 4); take(h->nms_bucket2, need); take(h->nms_sbox2, need * 4);
    drained = false;
    bool zero_ctr = false;
    for (DevBuf<int32_t>& b : h->nms_seg) zero_ctr = take(b, need_seg);          // ctr, the last one: >= 2 * B ints
    if (zero_ctr) rc = (int)hipMemsetAsync(h->nms_seg[9], 0, need_seg * sizeof(int32_t), h->stream);
    drained = false;
    take(h->nms_matrix, m_stride * B);
    drained = false;
    if (take(h->nms_pre_sync, need_ps)) rc = (int)hipMemsetAsync(h->nms_pre_sync, 0, need_ps * sizeof(unsigned long long), h->stream);
    NmsWork& w = h->nms;
    w.bucket = h->nms_bucket; w.keep = h->nms_keep; w.sbox = h->nms_sbox; w.bucket2 = h->nms_bucket2; w.sbox2 = h->nms_sbox2;
    int32_t** const seg[10] = {&w.seg_count, &w.seg_off, &w.tile_off, &w.large_list, &w.seg_count2, &w.tile_off2, &w.seg_order, &w.seg_sparse, &w.work_off, &w.ctr};
    for (int i = 0; i < 10; ++i) *seg[i] = h->nms_seg[i];
    w.matrix = h->nms_matrix; w.pre_sync = h->nms_pre_sync;
    w.matrix_stride = m_stride;
    w.large_cap = (N / 1024 + 1) < C ? (N / 1024 + 1) : C;       // at most N/1024 segments can exceed 1024 items
    if (moved) drop_graphs(h);
    if (rc) return fail(h, "NMS scratch for %d x %d candidates: %s", B, N, hipGetErrorString((hipError_t)rc));
    return 0;
}

// the NMS scratch (the WBF route starts with its bucket + sort) plus weighted box fusion's own arrays, owned the same way
int ensure_wbf(yn_handle* h, int B, int N, int C)
{
    if (ensure_post(h, B, N, C)) return 1;
    const size_t need = (size_t)B * N;
    int rc = 0;
    bool drained = false;
    auto take = [&](auto& buf, size_t n) {
        if (rc || n <= buf.cap()) return;
        if (!drained) { rc = (int)hipStreamSynchronize(h->stream); drained = true; }
        if (!rc) rc = buf.reserve(n);
    };
    take(h->wbf_box, need * 4); take(h->wbf_score, need); take(h->wbf_ofb, need * 4); take(h->wbf_op, need * 4); take(h->wbf_os, need);
    take(h->wbf_votes, need); take(h->wbf_index, need); take(h->wbf_on, need); take(h->wbf_ofounder, need);
    h->wbf = WbfWork{h->wbf_box, h->wbf_score, h->wbf_votes, h->wbf_index, h->wbf_ofb, h->wbf_op, h->wbf_os, h->wbf_on, h->wbf_ofounder};
    if (rc) return fail(h, "weighted box fusion scratch for %d x %d rows: %s", B, N, hipGetErrorString((hipError_t)rc));
    return 0;
}

// the NMS scratch (the Soft-NMS route starts with its bucket + sort) plus Soft-NMS's two score arrays; yn_infer captures them in its graphs
int ensure_soft(yn_handle* h, int B, int N, int C)
{
    if (ensure_post(h, B, N, C)) return 1;
    const size_t need = (size_t)B * N;
    int rc = 0;
    bool moved = false, drained = false;
    auto take = [&](auto& buf, size_t n) {
        if (rc || n <= buf.cap()) return;
        if (!drained) { rc = (int)hipStreamSynchronize(h->stream); drained = true; }
        if (!rc) rc = buf.reserve(n, 0, &moved);
    };
    take(h->soft_score, need); take(h->soft_spill, need);
    h->soft = SoftWork{h->soft_score, h->soft_spill};
    if (moved) drop_graphs(h);
    if (rc) return fail(h, "Soft-NMS scratch for %d x %d rows: %s", B, N, hipGetErrorString((hipError_t)rc));
    return 0;
}

// the parameter checks every Soft-NMS entry shares; lo = the smallest method the entry takes (YN_SOFT_OFF for the setters, YN_SOFT_HARD for a merge)
int soft_params(yn_handle* h, const char* who, int lo, int method, float sigma, float score_floor)
{
    if (method < lo || method > YN_SOFT_GAUSSIAN)
        return fail(h, "%s: method %d is not %sYN_SOFT_HARD (1), YN_SOFT_LINEAR (2) or YN_SOFT_GAUSSIAN (3)", who, method, lo == YN_SOFT_OFF ? "YN_SOFT_OFF (0), " : "");
    if (!(sigma > 0.0f) || sigma > 3.4028234e38f) return fail(h, "%s: sigma is %g (it must be positive and finite)", who, (double)sigma);
    if (!(score_floor >= 0.0f) || score_floor > 3.4028234e38f) return fail(h, "%s: score_floor is %g (it must be 0 or more and finite)", who, (double)score_floor);
    return 0;
}
static_assert(YN_SOFT_HARD == ynk::SOFT_HARD && YN_SOFT_LINEAR == ynk::SOFT_LINEAR && YN_SOFT_GAUSSIAN == ynk::SOFT_GAUSSIAN, "Soft-NMS methods (yn_internal.h)");

int ensure_heads(yn_handle* h, int B)
{
    const int hld = (h->head_ch + 3) & ~3;                  // internal heads: rows padded to 16 bytes => float4 stores
    const size_t need = (size_t)B * (h->grid.hw[0] + h->grid.hw[1] + h->grid.hw[2]) * hld + 256;      // + 1024 bytes of slack
    bool moved = false;
    int rc = 0;
    if (need > h->heads_buf.cap()) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        rc = h->heads_buf.reserve(need, 0, &moved);
    }
    // re-derive the split for the current grid
    h->heads_int[0] = h->heads_buf;
    h->heads_int[1] = h->heads_int[0] + (size_t)B * h->grid.hw[0] * hld;
    h->heads_int[2] = h->heads_int[1] + (size_t)B * h->grid.hw[1] * hld;
    if (moved) drop_graphs(h);
    if (rc) return fail(h, "raw head tensors for %d images: %s", B, hipGetErrorString((hipError_t)rc));
    return 0;
}

// ---- profiling brackets ---------------------------------------------------------------------------
hipEvent_t take_event(yn_handle* h)
{
    if (h->event_next == h->event_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        h->event_pool.push_back(e);
    }
    return h->event_pool[h->event_next++];
}

struct Bracket {
    yn_handle* h;
    bool on;
    Bracket(yn_handle* h_, const std::string& name, double flops, double bytes) : h(h_), on(h_->profiling)
    {
        if (!on) return;
        ProfRec r;
        r.name = name; r.flops = flops; r.bytes = bytes;
        r.e0 = take_event(h); r.e1 = take_event(h);
        (void)hipEventRecord(r.e0, h->cur);
        h->prof.push_back(r);
    }
    void cancel() { if (on) { h->prof.pop_back(); h->event_next -= 2; on = false; } }
    ~Bracket()
    {
        if (!on) return;
        (void)hipEventRecord(h->prof.back().e1, h->cur);
        h->prof.back().kernel = last_kernel_name();
    }
};

// ---- layer launchers ------------------------------------------------------------------------------
const Layer& L(yn_handle* h, const std::string& name) { return h->layers[h->by_name.at(name)]; }

// Pick the fastest tile configuration for this (shape, strides) by timing every instantiated one on the
// handle's stream (all configurations are bit-identical, so this only affects speed).  Never runs during capture.
int tune_pw(yn_handle* h, GemmArgs a)
{
    if (h->force_pw_cfg >= 0) return h->force_pw_cfg;
    if (!h->autotune) return -1;
    // the candidates: the split-f16 family for a layer that carries split packs, else the f32-MFMA family (each bit-identical inside)
    const int c_lo = a.Wsh ? pw_f32_config_count() : 0, c_hi = a.Wsh ? pw_config_count() - (h->pw_pipe ? 0 : 1) : pw_f32_config_count();   // (pw_pipe_kernel is the last index)
    // one table per process, shared by every handle (bench.py runs four per GPU: the layer shapes are timed once, not four times)
    const std::vector<int> key = {h->cfg.device, a.M, a.K, a.N, a.Npad, a.act, a.in_ld, a.in_off, a.out_ld, a.out_off, a.pass ? 1 : 0, a.Wsh ? 1 : 0, h->pw_pipe ? 1 : 0};
    {
        std::lock_guard<std::mutex> lk(g_tune_mutex);
        auto it = g_pw_tuned.find(key);
        if (it != g_pw_tuned.end()) return it->second;
    }
    if (h->profiling) return -1;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->cur, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return -1;
    if (!h->tune_e0) { (void)hipEventCreate(&h->tune_e0); (void)hipEventCreate(&h->tune_e1); }
    int best = -1;
    float best_ms = 1e30f;
    // two rounds over all candidates, minimum per candidate; every bracket spans >= ~300 us of launches (5...40 of them): a single
    // short bracket is noisy enough (clock ramp, a neighbour stream's kernel) to pick a tile 1.5x slower than the best one, and the
    // named workloads then moved by +-10 % from run to run
    int reps = 5;
    {
        a.cfg = c_lo;
        launch_pw(a, h->cur);
        (void)hipEventRecord(h->tune_e0, h->cur);
        launch_pw(a, h->cur); launch_pw(a, h->cur);
        (void)hipEventRecord(h->tune_e1, h->cur);
        float ms2 = 0.0f;
        if (hipEventSynchronize(h->tune_e1) != hipSuccess) return -1;
        (void)hipEventElapsedTime(&ms2, h->tune_e0, h->tune_e1);
        const float per = ms2 > 0.0f ? ms2 * 0.5f : 0.02f;
        reps = (int)(0.3f / per);
        reps = reps < 5 ? 5 : (reps > 40 ? 40 : reps);
    }
    for (int round = 0; round < 2; ++round) {
        for (int c = c_lo; c < c_hi; ++c) {
            a.cfg = c;
            launch_pw(a, h->cur);                           // warm-up
            (void)hipEventRecord(h->tune_e0, h->cur);
            for (int r = 0; r < reps; ++r) launch_pw(a, h->cur);
            (void)hipEventRecord(h->tune_e1, h->cur);
            if (hipEventSynchronize(h->tune_e1) != hipSuccess) return -1;
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, h->tune_e0, h->tune_e1);
            if (ms < best_ms) { best_ms = ms; best = c; }
        }
    }
    if (hipGetLastError() != hipSuccess) return -1;
    {
        std::lock_guard<std::mutex> lk(g_tune_mutex);
        g_pw_tuned[key] = best;
    }
    return best;
}

GemmArgs pw_args(yn_handle* h, const Layer& l, const float* in, int in_ld, int in_off, long M,
                 float* out, int out_ld, int out_off, const float* pass, int pass_ld, int pass_off, int n_store = 0)
{
    GemmArgs a{};
    a.in = in; a.in_ld = in_ld; a.in_off = in_off;
    a.Wp = l.w_packed; a.bias = l.b_packed;
    a.out = out; a.out_ld = out_ld; a.out_off = out_off;
    a.pass = pass; a.pass_ld = pass_ld; a.pass_off = pass_off;
    a.M = (int)M; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = l.act;
    a.in_slack = (h->arena && (const char*)in >= h->arena && (const char*)in < h->arena + h->arena_bytes) ? 16 : 0;
    if (n_store > l.cout && n_store <= l.Npad) a.N = n_store;     // padded output row: the extra (zero-weight) columns are stored too
    if (!exact(h)) { a.Wsh = l.ws_hi; a.Wsl = l.ws_lo; }          // split-f16 MFMA family (fp32-class); exact_f32 / range fallback: the f32-MFMA kernels
    a.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
    a.cfg = -1;
    return a;
}

void run_pw(yn_handle* h, const Layer& l, const float* in, int in_ld, int in_off, long M,
            float* out, int out_ld, int out_off, const float* pass, int pass_ld, int pass_off, int n_store = 0)
{
    GemmArgs a = pw_args(h, l, in, in_ld, in_off, M, out, out_ld, out_off, pass, pass_ld, pass_off, n_store);
    a.cfg = tune_pw(h, a);
    Bracket br(h, l.name, 2.0 * M * l.cin * l.cout,
               4.0 * (M * (double)(l.cin + l.cout + (pass ? 2 * l.cout : 0)) + (double)l.cin * l.cout));
    launch_pw(a, h->cur);
}

void run_dw(yn_handle* h, const Layer& l, const float* in, int in_ld, int in_off, int B, int H, int W,
            float* out, int out_ld, int out_off)
{
    DwArgs a{};
    a.in = in; a.in_ld = in_ld; a.in_off = in_off; a.w = l.w_packed; a.bias = l.b_packed;
    a.out = out; a.out_ld = out_ld; a.out_off = out_off;
    a.B = B; a.H = H; a.W = W; a.C = l.cout; a.stride = l.stride; a.act = l.act;
    const double Mi = (double)B * H * W, Mo = (double)B * ((H - 1) / l.stride + 1) * ((W - 1) / l.stride + 1);
    Bracket br(h, l.name, 2.0 * Mo * 9 * l.cout, 4.0 * (Mi + Mo) * l.cout);
    launch_dw(a, h->cur);
}

// stride-1 ShuffleV2 unit (backbone/shufflenetv2.py:70-72): x [B,H,W,C] -> out [B,H,W,C] as pointwise -> depthwise ->
// pointwise with the concat+shuffle epilogue (t1, t2 scratch); the one-kernel-per-unit form is run_unit_chain below
void run_dwpw(yn_handle* h, const Layer& dw, const Layer& pw, const float* in, int in_ld, int in_off, int B, int H, int W,
              float* tmp, float* out, int out_ld, int out_off, const float* pass, int pass_ld, int pass_off);
void run_unit(yn_handle* h, const std::string& P, const float* x, int B, int H, int W, float* out, float* t1, float* t2)
{
    const Layer& pw1 = L(h, P + ".b2.pw1");
    const Layer& dw = L(h, P + ".b2.dw");
    const Layer& pw2 = L(h, P + ".b2.pw2");
    const int bf = pw1.cout, C = 2 * bf;
    const long M = (long)B * H * W;
    run_pw(h, pw1, x, C, bf, M, t1, bf, 0, nullptr, 0, 0);
    run_dwpw(h, dw, pw2, t1, bf, 0, B, H, W, t2, out, C, 0, x, C, 0);
}

// Units 1..R-1 of a stage as pw1(unit 1) + one unit_chain_kernel per unit.  oA = the stride-2 block's output [M][C] (unit 1's
// input), oB = a second [M][C] buffer (holds the two [M][bf] pass-through halves in flight), tA / tB = [M][bf] scratch.
// Returns 0 (nothing launched) when the chain is off, the map is too small or no instantiated tile covers the shape; 1 when
// the stage ran, *result = final [M][C]; -1 on an error (latched in the handle).
// dry: only answer whether the stage will run as a chain (nothing launched).  t1_ready: unit 1's pw1 output is already in tA (the stride-2
// unit's kernel computed it: down2_kernel's last phase)
int run_unit_chain(yn_handle* h, int stage, int R, float* oA, int B, int H, int W, int C, float* oB, float* tA, float* tB, float** result,
                   bool dry = false, bool t1_ready = false)
{
    if (!h->unit_chain) return 0;
    const int bf = C / 2;
    const long M = (long)B * H * W;
    // Stages 2 and 3 (bf <= 128) chain at every size: on one image's maps the 32-row tiles of unit_chain2_kernel run a unit in 12 - 16 us
    // against 8 + 6 + 8 for its three kernels (bs = 1: 0.620 -> 0.585 ms at 416 x 416, 0.757 -> 0.719 ms at 608 x 608).  Stage 4 (bf = 232) chained
    // from M = 4 096 pixels only while the chain kernel staged its weights through LDS (eight chunk rounds per GEMM: 32 + 30 + 19 us against 3 x 29 on
    // one image).  With the weights register-direct (round 4) the chain costs one image what its three launches did (0.5245 vs 0.5227 ms at 416,
    // 0.653-0.660 either way at 608; bs 2 / 4 / 8 / 16: 0.554 / 0.622 / 0.714 / 0.847 vs 0.548 / 0.617 / 0.718 / 0.850 ms) and is six launches
    // less: it chains at every size now.
    char nm[96];
    auto name = [&](int bi) { snprintf(nm, sizeof nm, "backbone.stage%d.%d", stage, bi); return std::string(nm); };
    {
        const Layer& pw1 = L(h, name(1) + ".b2.pw1");
        const Layer& dw = L(h, name(1) + ".b2.dw");
        if (pw1.cin != bf || pw1.cout != bf || dw.stride != 1) return 0;
        // every unit of the stage must be covered by an instantiated tile BEFORE anything is launched: the chain consumes its
        // input buffers, so there is no falling back half way (unit 1 reads x1 with ld = C, the others with ld = bf)
        for (int first = 0; first < 2; ++first) {
            ChainArgs q{};
            q.t1_ld = bf; q.x1_ld = first ? C : bf; q.out_ld = bf; q.bf = bf; q.Npad = L(h, name(1) + ".b2.pw2").Npad; q.M = (int)M;
            if (!exact(h)) q.Ws2h = L(h, name(1) + ".b2.pw2").ws_hi;
            if (!unit_chain_covers(q)) return 0;
            q.out_ld = C;
            if (!unit_chain_covers(q)) return 0;
        }
        if (dry) return 1;
        if (!t1_ready) run_pw(h, pw1, oA, C, bf, M, tA, bf, 0, nullptr, 0, 0);
    }
    float* pbuf[2] = {oB, oB + (size_t)M * bf};
    const float* x1 = oA;
    int x1_ld = C;
    float* final_out = R > 2 ? oA : oB;
    std::vector<ChainArgs> ua;
    for (int bi = 1; bi < R; ++bi) {
        const std::string P = name(bi);
        const bool last = bi == R - 1;
        const Layer& dw = L(h, P + ".b2.dw");
        const Layer& pw2 = L(h, P + ".b2.pw2");
        ChainArgs a{};
        a.t1 = tA; a.t1_ld = bf; a.t1_off = 0;
        a.x1 = x1; a.x1_ld = x1_ld; a.x1_off = 0;
        a.wdw = dw.w_packed; a.bdw = dw.b_packed; a.dw_act = dw.act;
        a.Wp2 = pw2.w_packed; a.b2 = pw2.b_packed; a.act2 = pw2.act;
        if (!exact(h)) { a.Ws2h = pw2.ws_hi; a.Ws2l = pw2.ws_lo; }
        if (!last) {
            const Layer& pw1n = L(h, name(bi + 1) + ".b2.pw1");
            a.Wp1n = pw1n.w_packed; a.b1n = pw1n.b_packed; a.act1n = pw1n.act;
            if (!exact(h)) { a.Ws1h = pw1n.ws_hi; a.Ws1l = pw1n.ws_lo; }
            a.out = pbuf[(bi - 1) & 1]; a.out_ld = bf; a.t1n = tB;
        } else {
            a.out = final_out; a.out_ld = C;
        }
        a.B = B; a.H = H; a.W = W; a.bf = bf; a.Npad = pw2.Npad; a.M = (int)M;
        a.pipe_mode = h->chain_pipe;
        a.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
        ua.push_back(a);
        x1 = a.out; x1_ld = bf;
        float* tmp = tA; tA = tB; tB = tmp;
    }
    // All but the last unit as ONE persistent launch (stage_pipe_kernel, kernels_stage.hip) where a form exists: the conditions of
    // unit_pipe_kernel (split-f16 family, ReLU pointwise / linear depthwise convs, dense inputs) + channel quads + enough tiles to walk
    int staged = 0;
    if (h->stage_fuse && !exact(h) && R - 2 >= 2 && R - 2 <= YN_STAGE_MAX && h->stage_sync) {
        StageArgs sa{};
        bool ok = true;
        double fl = 0, by = 0;
        for (int i = 0; i < R - 2 && ok; ++i) {
            const ChainArgs& q = ua[i];
            ok = q.Ws2h && q.Ws1h && q.dw_act == 0 && q.act2 == 1 && q.act1n == 1 && q.t1_ld == bf && q.t1_off == 0 && q.x1_off == 0 && (q.x1_ld & 3) == 0 &&
                 q.out_ld == bf && q.Npad == ((bf + 31) & ~31);
            StageUnit& u = sa.u[i];
            u.t1 = q.t1; u.x1 = q.x1; u.x1_ld = q.x1_ld; u.wdw = q.wdw; u.bdw = q.bdw; u.b2 = q.b2; u.b1n = q.b1n;
            u.Ws2h = q.Ws2h; u.Ws2l = q.Ws2l; u.Ws1h = q.Ws1h; u.Ws1l = q.Ws1l; u.out = q.out; u.t1n = q.t1n;
            fl += 2.0 * M * bf * (9.0 + 2.0 * bf);
            by += 4.0 * (4.0 * M * bf + 2.0 * bf * bf + 10.0 * bf);
        }
        sa.nunits = R - 2; sa.M = (int)M; sa.H = H; sa.W = W;
        sa.inv_w = 1.0f / (float)W; sa.inv_h = 1.0f / (float)H;
        sa.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
        sa.sync = h->stage_sync;
        const int min_tiles = h->stage_fuse == 2 ? 1 : 256;
        if (ok && launch_stage_pipe(sa, bf, h->stage_pub_early, min_tiles, h->stage_sync_bytes, h->cur, true)) {
            snprintf(nm, sizeof nm, "backbone.stage%d.1-%d.dw+pw2+pw1n", stage, R - 2);
            const std::string sname = nm;
            Bracket br(h, sname, fl, by);
            (void)launch_stage_pipe(sa, bf, h->stage_pub_early, min_tiles, h->stage_sync_bytes, h->cur);
            staged = R - 2;
        }
    }
    for (int bi = 1 + staged; bi < R; ++bi) {
        const std::string P = name(bi);
        const bool last = bi == R - 1;
        const ChainArgs& a = ua[bi - 1];
        Bracket br(h, P + (last ? ".dw+pw2" : ".dw+pw2+pw1n"), 2.0 * M * bf * (9.0 + bf + (last ? 0.0 : (double)bf)),
                   4.0 * (4.0 * M * bf + (last ? 1.0 : 2.0) * bf * bf + 10.0 * bf));
        if (!launch_unit_chain(a, h->cur)) {                 // cannot happen after the coverage check above
            br.cancel();
            fail(h, "unit chain: no tile for stage %d unit %d after the coverage check", stage, bi);
            return -1;                                         // never fall back here: the chain has consumed its input buffers
        }
    }
    *result = final_out;
    return 1;
}

void run_dwpw(yn_handle* h, const Layer& dw, const Layer& pw, const float* in, int in_ld, int in_off, int B, int H, int W,
              float* tmp, float* out, int out_ld, int out_off, const float* pass, int pass_ld, int pass_off)
{
    const int Ho = (H - 1) / dw.stride + 1, Wo = (W - 1) / dw.stride + 1;
    const long M = (long)B * Ho * Wo;                       // output pixels
    run_dw(h, dw, in, in_ld, in_off, B, H, W, tmp, dw.cout, 0);
    run_pw(h, pw, tmp, dw.cout, 0, M, out, out_ld, out_off, pass, pass_ld, pass_off);
}

void run_c3(yn_handle* h, const Layer& l, const float* in, const float* in2, int resample, int B, int H, int W, float* out)
{
    GemmArgs a{};
    a.in = in; a.in_ld = l.cin; a.in_off = 0; a.in2 = in2; a.resample = resample; a.H = H; a.W = W;
    a.Wp = l.w_packed; a.bias = l.b_packed; a.out = out; a.out_ld = l.cout; a.out_off = 0;
    a.M = B * H * W; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = l.act;
    a.cfg = -1;
    if (!exact(h)) { a.Wsh = l.ws_hi; a.Wsl = l.ws_lo; }         // split-f16 MFMA path (fp32-class); exact_f32 / range fallback: the f32-MFMA kernel
    a.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
    const double M = (double)a.M;
    const double in2px = resample == 1 ? M / 4 : (resample == 2 ? M * 4 : 0);
    Bracket br(h, l.name, 2.0 * M * 9 * l.cin * l.cout, 4.0 * ((M + in2px) * l.cin + M * l.cout + 9.0 * l.cin * l.cout));
    launch_conv3x3(a, h->cur);
}

// ---- grouped launches (Group<>, yn_internal.h): the same layer of the three detection heads / the three laterals as ONE launch ----
bool run_pw_group(yn_handle* h, const Layer* const l[], GemmArgs a[], int n, const char* name)
{
    // the tile configuration is timed for the GROUP (one launch of every split configuration, as tune_pw does for a single layer): the
    // best tile of the largest problem can leave a small-M / long-K member with a handful of serial workgroups (the laterals: K = 464 on
    // 5 408 pixels rode for 57 us on the 128-row tile of the 86 528-pixel member).  Every split configuration gives the same bits.
    a[0].cfg = -1;
    if (h->autotune && h->force_pw_cfg < 0) {
        std::vector<int> key = {h->cfg.device, -n};
        for (int p = 0; p < n; ++p) { key.push_back(a[p].M); key.push_back(a[p].K); key.push_back(a[p].N); key.push_back(a[p].in_ld); key.push_back(a[p].out_ld); }
        bool found = false;
        {
            std::lock_guard<std::mutex> lk(g_tune_mutex);
            auto it = g_pw_tuned.find(key);
            if (it != g_pw_tuned.end()) { a[0].cfg = it->second; found = true; }
        }
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (!found && !h->profiling && hipStreamIsCapturing(h->cur, &st) == hipSuccess && st == hipStreamCaptureStatusNone) {
            if (!h->tune_e0) { (void)hipEventCreate(&h->tune_e0); (void)hipEventCreate(&h->tune_e1); }
            int best = -1;
            float best_ms = 1e30f;
            for (int round = 0; round < 2; ++round)
                for (int c = pw_f32_config_count(); c < pw_config_count(); ++c) {
                    if (c == pw_config_count() - 1 && !pw_pipe_group_candidate(a, n)) continue;      // the persistent form: only where it has a form and its workgroups walk
                    if (!launch_pw_group(a, n, c, h->cur)) continue;                 // warm-up
                    (void)hipEventRecord(h->tune_e0, h->cur);
                    for (int r = 0; r < 5; ++r) (void)launch_pw_group(a, n, c, h->cur);
                    (void)hipEventRecord(h->tune_e1, h->cur);
                    if (hipEventSynchronize(h->tune_e1) != hipSuccess) { best = -1; break; }
                    float ms = 0.0f;
                    (void)hipEventElapsedTime(&ms, h->tune_e0, h->tune_e1);
                    if (ms < best_ms) { best_ms = ms; best = c; }
                }
            if (best >= 0) {
                std::lock_guard<std::mutex> lk(g_tune_mutex);
                g_pw_tuned[key] = best;
                a[0].cfg = best;
            }
        }
    } else if (h->force_pw_cfg >= 0) a[0].cfg = h->force_pw_cfg;
    double fl = 0, by = 0;
    for (int p = 0; p < n; ++p) {
        fl += 2.0 * a[p].M * l[p]->cin * l[p]->cout;
        by += 4.0 * (a[p].M * (double)(l[p]->cin + l[p]->cout) + (double)l[p]->cin * l[p]->cout);
    }
    Bracket br(h, name, fl, by);
    if (launch_pw_group(a, n, a[0].cfg, h->cur)) return true;
    br.cancel();
    return false;
}

void run_dw_group(yn_handle* h, const Layer* const l[], DwArgs a[], int n, const char* name)
{
    double fl = 0, by = 0;
    for (int p = 0; p < n; ++p) {
        const double M = (double)a[p].B * a[p].H * a[p].W;
        fl += 2.0 * M * 9 * l[p]->cout;
        by += 4.0 * 2 * M * l[p]->cout;
    }
    Bracket br(h, name, fl, by);
    launch_dw_group(a, n, h->cur);
}

// ---- fork / join of independent kernel chains onto side streams (also legal inside stream capture) ----
hipEvent_t fj_event(yn_handle* h)
{
    if (h->fj_events.size() < 32) {
        hipEvent_t e;
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        h->fj_events.push_back(e);
        return e;
    }
    return h->fj_events[h->fj_next++ % h->fj_events.size()];
}
bool side_ok(yn_handle* h)
{
    if (!h->multi_stream || h->profiling || h->stream == nullptr) return false;
    for (int k = 0; k < 2; ++k)
        if (!h->side[k] && hipStreamCreateWithFlags(&h->side[k], hipStreamNonBlocking) != hipSuccess) return false;
    return true;
}
// side stream k picks up after everything issued so far on the main stream; subsequent run_* target it
void fork_to(yn_handle* h, int k)
{
    if (!side_ok(h)) return;
    hipEvent_t e = fj_event(h);
    (void)hipEventRecord(e, h->stream);
    (void)hipStreamWaitEvent(h->side[k], e, 0);
    h->cur = h->side[k];
}
void back_to_main(yn_handle* h) { h->cur = h->stream; }
// the main stream waits for everything issued so far on side stream k
void join_from(yn_handle* h, int k)
{
    if (!h->side[k] || !side_ok(h)) return;
    hipEvent_t e = fj_event(h);
    (void)hipEventRecord(e, h->side[k]);
    (void)hipStreamWaitEvent(h->stream, e, 0);
}

static GemmArgs head_final_args(yn_handle* h, const Layer& l, const float* in, long M)
{
    GemmArgs a{};
    a.in = in; a.in_ld = NECK; a.in_off = 0;
    a.Wp = l.w_packed; a.bias = l.b_packed;
    a.M = (int)M; a.K = l.cin; a.N = l.cout; a.Npad = l.Npad; a.act = l.act;
    a.Wsh = l.ws_hi; a.Wsl = l.ws_lo;
    a.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
    a.cfg = -1;
    return a;
}

// Whether a forward over B images hands the last head conv and the candidate decode to one kernel (head_decode*_kernel / head_tail_group_kernel):
// the handle's switches, what the layers' packs allow, and the size rule.  want = the caller decodes at all (yn_infer, yn_op_head_tail).
static bool head_fuse_all(yn_handle* h, int B, bool want)
{
    char nm[96];
    const long M3 = (long)B * h->grid.hw[0];
    bool fuse_all = want && h->fuse_decode && !exact(h);
    for (int hd = 0; hd < 3 && fuse_all; ++hd) {
        snprintf(nm, sizeof nm, "head_det_%d.4", hd + 1);
        fuse_all = head_decode_supported(head_final_args(h, L(h, nm), nullptr, (long)B * h->grid.hw[hd]), h->grid);
    }
    // small batches: three 16 us fused launches against three 10 us GEMMs + one 7 us decode (bs = 1) - the fusion pays from the
    // traffic it removes, i.e. when the stride-8 head is large (bs >= 4 at 416x416); yn_fuse_decode(2) forces it (tests)
    // ... unless the wider fusion applies (head_tail_group_kernel: layers .2-.4 + decode as ONE launch instead of three: bs = 1 0.602 -> 0.593 ms)
    bool tail_possible = false;
    if (fuse_all && h->tail_fuse && h->group_launch && h->grid.C > 32) {
        const GemmArgs gf = head_final_args(h, L(h, "head_det_1.4"), nullptr, M3);
        tail_possible = gf.Npad > 128 && gf.Npad <= 256;
    }
    if (h->fuse_decode_mode != 2 && M3 < 8192 && !tail_possible) fuse_all = false;
    return fuse_all;
}

// Layer k of the three heads as ONE grouped launch (hl = the three heads' layers): depthwise, pointwise, or a depthwise + pointwise pair
// as one kernel (the depthwise output never reaches memory).  src_feat, when given, replaces src_own (layer .0 reads the pyramid levels).
static bool head_dw_layer(yn_handle* h, const Layer* const hl[3], int B, const float* const src_own[3], const float* const src_feat[3], float* const dst[3], const char* name)
{
    DwArgs d[3];
    for (int hd = 0; hd < 3; ++hd) {
        const Layer& l = *hl[hd];
        const int H = h->grid.h[hd], W = h->grid.w[hd];
        d[hd] = DwArgs{};
        d[hd].in = src_feat ? src_feat[hd] : src_own[hd]; d[hd].in_ld = NECK; d[hd].in_off = 0; d[hd].w = l.w_packed; d[hd].bias = l.b_packed;
        d[hd].out = dst[hd]; d[hd].out_ld = NECK; d[hd].out_off = 0;
        d[hd].B = B; d[hd].H = H; d[hd].W = W; d[hd].C = l.cout; d[hd].stride = l.stride; d[hd].act = l.act;
    }
    if (!dw_group_ok(d, 3)) return false;
    run_dw_group(h, hl, d, 3, name);
    return true;
}

static bool head_pw_layer(yn_handle* h, const Layer* const hl[3], int B, const float* const src[3], float* const dst[3], int dst_ld, int n_store, const char* name)
{
    GemmArgs g3[3];
    for (int hd = 0; hd < 3; ++hd) {
        g3[hd] = pw_args(h, *hl[hd], src[hd], NECK, 0, (long)B * h->grid.hw[hd], dst[hd], dst_ld, 0, nullptr, 0, 0, n_store);
    }
    return run_pw_group(h, hl, g3, 3, name);
}

static bool head_dwpw_layer(yn_handle* h, const Layer* const hld[3], const Layer* const hlp[3], int B, const float* const src_own[3], const float* const src_feat[3],
                            float* const dst[3], const char* name)
{
    DwPwArgs q[3];
    double fl = 0, by = 0;
    for (int hd = 0; hd < 3; ++hd) {
        const Layer &ld = *hld[hd], &lp = *hlp[hd];
        const int H = h->grid.h[hd], W = h->grid.w[hd];
        q[hd] = DwPwArgs{};
        q[hd].in = src_feat ? src_feat[hd] : src_own[hd];
        q[hd].wdw = ld.w_packed; q[hd].bdw = ld.b_packed; q[hd].dw_act = ld.act;
        q[hd].Wh = lp.ws_hi; q[hd].Wl = lp.ws_lo; q[hd].bias = lp.b_packed; q[hd].act = lp.act; q[hd].Npad = lp.Npad;
        q[hd].out = dst[hd]; q[hd].B = B; q[hd].H = H; q[hd].W = W; q[hd].C = ld.cout;
        q[hd].ovf = h->range_flags ? h->range_flags + 1 : nullptr;
        if (ld.stride != 1 || ld.cout != NECK || lp.cin != NECK || lp.cout != NECK) return false;
        const double M = (double)B * H * W;
        fl += 2.0 * M * NECK * (9.0 + NECK);
        by += 4.0 * (2.0 * M * NECK + (double)NECK * NECK);
    }
    if (!dwpw_group_ok(q, 3)) return false;
    Bracket br(h, name, fl, by);
    launch_dwpw_group(q, 3, h->cur);
    return true;
}

// layers .2 + .3 + .4 + the decode of the three heads as ONE grouped kernel (head_tail_group_kernel): layer .3's output never reaches memory
static bool head_tail_layer(yn_handle* h, const Layer* const hl2[3], const Layer* const hl3[3], const Layer* const hl4[3], int B, const float* const src[3], bool fuse_all)
{
    if (!fuse_all || !h->tail_fuse) return false;
    HeadTailArgs q[3];
    double fl = 0, by = 0;
    for (int hd = 0; hd < 3; ++hd) {
        const Layer &ld = *hl2[hd], &lp = *hl3[hd], &lf = *hl4[hd];
        const int H = h->grid.h[hd], W = h->grid.w[hd];
        if (ld.stride != 1 || ld.cout != NECK || lp.cin != NECK || lp.cout != NECK || lp.Npad != NECK || lf.cin != NECK || NECK != 96 || !lf.ws_hi) return false;
        const GemmArgs gf = head_final_args(h, lf, src[hd], (long)B * H * W);
        if (gf.act != 0 || gf.pass) return false;
        q[hd] = HeadTailArgs{};
        q[hd].in = src[hd]; q[hd].wdw = ld.w_packed; q[hd].bdw = ld.b_packed; q[hd].dw_act = ld.act;
        q[hd].Wh = lp.ws_hi; q[hd].Wl = lp.ws_lo; q[hd].bias = lp.b_packed; q[hd].act = lp.act;
        q[hd].Wfh = gf.Wsh; q[hd].Wfl = gf.Wsl; q[hd].fbias = gf.bias; q[hd].Npad = gf.Npad;
        q[hd].B = B; q[hd].H = H; q[hd].W = W;
        q[hd].ovf = h->range_flags ? h->range_flags + 1 : nullptr;
        const double M = (double)B * H * W;
        fl += 2.0 * M * NECK * (9.0 + NECK) + 2.0 * M * lf.cin * lf.cout;
        by += 4.0 * (M * NECK + (double)NECK * NECK + (double)lf.cin * lf.cout + 6.0 * M * h->grid.A);
    }
    if (!head_tail_ok(q, 3, h->grid)) return false;
    Bracket br(h, "head_det_*.2+3+4+decode", fl, by);
    launch_head_tail_group(q, 3, h->grid, h->cfg.conf_thresh, h->cand_boxes, h->cand_scores, h->cand_cls, h->cur);
    return true;
}

// The detection heads from the output of their layer .1 (src) to the end, on h->cur: layers .2 + .3 (scratch hA, output hC), then layer .4
// into heads[] (row stride head_ld) or, with fuse_all, layer .4 + the candidate decode into h->cand_*.  hd = 0..2: that head with its own
// launches; hd < 0: the three heads with grouped launches (the split-f16 family: the caller has checked the packs).  yn_infer's forward and
// yn_op_head_tail both come through here.
static int run_head_tail(yn_handle* h, int hd, int B, const float* const src[3], float* const hA[3], float* const hC[3], float* const heads[3], int head_ld, bool fuse_all)
{
    char nm[96];
    if (hd >= 0) {
        const int H = h->grid.h[hd], W = h->grid.w[hd];
        const long M = (long)B * H * W;
        snprintf(nm, sizeof nm, "head_det_%d", hd + 1);
        const std::string P = nm;
        run_dwpw(h, L(h, P + ".2"), L(h, P + ".3"), src[hd], NECK, 0, B, H, W, hA[hd], hC[hd], NECK, 0, nullptr, 0, 0);
        const Layer& lf = L(h, P + ".4");
        if (fuse_all) {
            GemmArgs a = head_final_args(h, lf, hC[hd], M);
            Bracket br(h, lf.name + "+decode", 2.0 * M * lf.cin * lf.cout, 4.0 * (M * (double)lf.cin + (double)lf.cin * lf.cout + 6.0 * M * h->grid.A));
            launch_head_decode(a, h->grid, hd, h->cfg.conf_thresh, h->cand_boxes, h->cand_scores, h->cand_cls, h->cur);
        } else {
            run_pw(h, lf, hC[hd], NECK, 0, M, heads[hd], head_ld, 0, nullptr, 0, 0, head_ld);
        }
        return 0;
    }
    const Layer* hl[3][3];
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) {
            snprintf(nm, sizeof nm, "head_det_%d.%d", d + 1, k + 2);
            hl[k][d] = &L(h, nm);
        }
    if (head_tail_layer(h, hl[0], hl[1], hl[2], B, src, fuse_all)) return 0;
    bool ok = head_dwpw_layer(h, hl[0], hl[1], B, src, nullptr, hC, "head_det_*.2+3") ||
              (head_dw_layer(h, hl[0], B, src, nullptr, hA, "head_det_*.2") && head_pw_layer(h, hl[1], B, hA, hC, NECK, 0, "head_det_*.3"));
    if (ok) {
        if (fuse_all) {
            GemmArgs g3[3];
            double fl = 0, by = 0;
            for (int d = 0; d < 3; ++d) {
                const long M = (long)B * h->grid.hw[d];
                g3[d] = head_final_args(h, *hl[2][d], hC[d], M);
                fl += 2.0 * M * hl[2][d]->cin * hl[2][d]->cout;
                by += 4.0 * (M * (double)hl[2][d]->cin + (double)hl[2][d]->cin * hl[2][d]->cout + 6.0 * M * h->grid.A);
            }
            Bracket br(h, "head_det_*.4+decode", fl, by);
            launch_head_decode_group(g3, 3, h->grid, h->cfg.conf_thresh, h->cand_boxes, h->cand_scores, h->cand_cls, h->cur);
        } else {
            ok = head_pw_layer(h, hl[2], B, hC, heads, head_ld, head_ld, "head_det_*.4");
        }
    }
    if (!ok) return fail(h, "grouped head launch: unsupported layer layout");
    return 0;
}

// true when every GEMM-shaped head layer carries split-f16 packs, which the grouped head launches need
static bool heads_groupable(yn_handle* h)
{
    if (!h->group_launch || exact(h)) return false;
    char nm[96];
    for (int k = 0; k < 5; ++k)
        for (int hd = 0; hd < 3; ++hd) {
            snprintf(nm, sizeof nm, "head_det_%d.%d", hd + 1, k);
            if ((k == 1 || k == 3 || k == 4) && !L(h, nm).ws_hi) return false;
        }
    return true;
}

// The network: x NCHW [B,3,H,W] (the grid's canvas; H = W = S on a square grid) -> three NHWC head tensors.
// fuse_decode: the last conv of each head runs as head_decode_kernel (candidates written straight into h->cand_*, raw heads not stored);
// *fused reports whether all three heads took that path (else the caller runs decode_kernel on the raw heads).
int run_network(yn_handle* h, const float* x, int B, float* const heads[3], int head_ld, bool fuse_decode = false, bool* fused = nullptr)
{
    const int GH = h->grid.H, GW = h->grid.W;
    h->arena_used = 0;
    h->cur = h->stream;
#define TAKE(var, floats)                                                                   \
    float* var = arena_take(h, (size_t)(floats));                                           \
    if (!var) return fail(h, "activation arena exhausted (%zu bytes)", h->arena_bytes)
    const int H1 = GH / 2, W1 = GW / 2, H2 = GH / 4, W2 = GW / 4;
    TAKE(a0, (size_t)B * H1 * W1 * 24);
    TAKE(a1, (size_t)B * H2 * W2 * 24);
    {
        // stem conv + maxpool in one kernel: the [B,H/2,W/2,24] conv activation stays in LDS (a0 is unused)
        const Layer& l = L(h, "stem");
        const double Mo = (double)B * H1 * W1;
        Bracket br(h, "stem+maxpool", 2.0 * Mo * 27 * 24, 4.0 * ((double)B * 3 * GH * GW + (double)B * H2 * W2 * 24));
        launch_stem_pool(x, B, GH, GW, l.w_packed, l.b_packed, l.cout, l.act, a1, h->cur);
    }
    const float* cur = a1;
    int curC = 24, curH = H2, curW = W2;
    const float* cfeat[3];
    char nm[96];
    for (int si = 0; si < 3; ++si) {
        const int C = h->stage_ch[si], bf = C / 2, Ho = curH / 2, Wo = curW / 2;
        const long Mi = (long)B * curH * curW, Mo = (long)B * Ho * Wo;
        TAKE(tdw1, Mo * curC);
        TAKE(tb1, Mo * bf);
        TAKE(t1, Mi * bf);
        TAKE(t2, Mo * bf);
        TAKE(oA, Mo * C);
        TAKE(oB, Mo * C);
        snprintf(nm, sizeof nm, "backbone.stage%d.0", si + 2);
        const std::string P0 = nm;
        bool down_chained = false;                          // the stride-2 unit's kernel has also produced unit 1's pw1 output (in t2)
        // stride-2 block: backbone/shufflenetv2.py:73-74
        {
            // the whole unit as ONE kernel where its tile fits (cin <= 32, bf <= 64: stage 2, whose pw1 output is the largest tensor of the
            // network): branch 2 = pw1 -> depthwise s2 -> pw2, branch 1 = depthwise s2 -> pw, concat + shuffle in the store
            const Layer &lp1 = L(h, P0 + ".b2.pw1"), &ldw = L(h, P0 + ".b2.dw"), &lp2 = L(h, P0 + ".b2.pw2");
            const Layer &l1d = L(h, P0 + ".b1.dw"), &l1p = L(h, P0 + ".b1.pw");
            DownArgs d{};
            d.x = cur; d.cin = curC;
            d.W1h = lp1.ws_hi; d.W1l = lp1.ws_lo; d.b1 = lp1.b_packed; d.act1 = lp1.act; d.Npad1 = lp1.Npad;
            d.wdw = ldw.w_packed; d.bdw = ldw.b_packed; d.dw_act = ldw.act;
            d.W2h = lp2.ws_hi; d.W2l = lp2.ws_lo; d.b2 = lp2.b_packed; d.act2 = lp2.act; d.Npad2 = lp2.Npad;
            d.wdw1 = l1d.w_packed; d.bdw1 = l1d.b_packed; d.dw1_act = l1d.act;
            d.W3h = l1p.ws_hi; d.W3l = l1p.ws_lo; d.b3 = l1p.b_packed; d.act3 = l1p.act; d.Npad3 = l1p.Npad;
            d.out = oA; d.B = B; d.H = curH; d.W = curW; d.bf = bf;
            d.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
            const bool use_down = h->down_fuse && !exact(h) && lp1.cin == curC && lp1.cout == bf && lp2.cin == bf && lp2.cout == bf && ldw.stride == 2 &&
                                  l1d.stride == 2 && l1d.cout == curC && l1p.cin == curC && l1p.cout == bf && down_unit_covers(d);
            Down2Args d2{};
            d2.x = cur; d2.cin = curC; d2.y1 = t1;
            d2.wdw = ldw.w_packed; d2.bdw = ldw.b_packed; d2.dw_act = ldw.act;
            d2.W2h = lp2.ws_hi; d2.W2l = lp2.ws_lo; d2.b2 = lp2.b_packed; d2.act2 = lp2.act;
            d2.wdw1 = l1d.w_packed; d2.bdw1 = l1d.b_packed; d2.dw1_act = l1d.act;
            d2.W3h = l1p.ws_hi; d2.W3l = l1p.ws_lo; d2.b3 = l1p.b_packed; d2.act3 = l1p.act;
            d2.out = oA; d2.B = B; d2.H = curH; d2.W = curW; d2.bf = bf; d2.Npad = lp2.Npad;
            d2.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
            const bool use_down2 = !use_down && h->down_fuse && !exact(h) && lp1.ws_hi && lp1.cin == curC && lp1.cout == bf && lp2.cin == bf && lp2.cout == bf &&
                                   ldw.stride == 2 && ldw.cout == bf && l1d.stride == 2 && l1d.cout == curC && l1p.cin == curC && l1p.cout == bf && l1p.Npad == lp2.Npad &&
                                   down2_covers(d2);
            // when the stride-1 units behind it run as a chain, the kernel also computes unit 1's pw1 (on channels [bf, 2bf) of its own output)
            // ... in the launch-latency regime only (at most 64 tiles of 32 pixels: one to a few images - one 608 x 608 image saves two 10-15 us
            // launches).  Beyond that the extra k-steps stream their weights at the CU's L1 rate (each 32-row workgroup pulls the whole
            // matrix): 42 us against 30 + 13 at stage 3 (676 tiles), 58 against 34 + 17 at stage 4 (169 tiles) of a 32-image batch.
            const bool next_pays = Mo <= 32 * 64;
            if (use_down2 && next_pays && STAGE_REP[si] > 1 && run_unit_chain(h, si + 2, STAGE_REP[si], oA, B, Ho, Wo, C, oB, t2, t1, nullptr, true) == 1) {
                snprintf(nm, sizeof nm, "backbone.stage%d.1.b2.pw1", si + 2);
                const Layer& l1n = L(h, nm);
                if (l1n.ws_hi && l1n.cin == bf && l1n.cout == bf && l1n.Npad == lp2.Npad) {
                    d2.W1nh = l1n.ws_hi; d2.W1nl = l1n.ws_lo; d2.b1n = l1n.b_packed; d2.act1n = l1n.act; d2.t1n = t2;
                    down_chained = true;
                }
            }
            if (use_down) {
                Bracket br(h, P0 + ".unit", 2.0 * (Mi * curC * bf + Mo * bf * (9.0 + bf) + Mo * curC * (9.0 + bf)),
                           4.0 * (Mi * (double)curC + 2.0 * Mo * bf + 2.0 * (double)curC * bf + (double)bf * bf));
                launch_down_unit(d, h->cur);
            } else if (use_down2) {
                // stages 3 / 4 (cin = bf = 116 / 232): pw1 as a GEMM launch, everything behind it - both depthwise convs, both pointwise convs,
                // concat + shuffle - as one kernel (down2_kernel): two launches instead of five
                run_pw(h, lp1, cur, curC, 0, Mi, t1, bf, 0, nullptr, 0, 0);
                const double nx = down_chained ? 1.0 : 0.0;
                Bracket br(h, P0 + (down_chained ? ".dw+pw2|b1+pw1n" : ".dw+pw2|b1"), 2.0 * (Mo * bf * (9.0 + bf) + Mo * curC * (9.0 + bf) + nx * Mo * bf * bf),
                           4.0 * (Mi * (double)(curC + bf) + (2.0 + nx) * Mo * bf + (double)curC * bf + (1.0 + nx) * bf * bf));
                launch_down2(d2, h->cur);
            } else {
        fork_to(h, 0);                                      // branch1 and branch2 only meet in the fused cat+shuffle
        {
            run_dw(h, L(h, P0 + ".b1.dw"), cur, curC, 0, B, curH, curW, tdw1, curC, 0);
            run_pw(h, L(h, P0 + ".b1.pw"), tdw1, curC, 0, Mo, tb1, bf, 0, nullptr, 0, 0);
            back_to_main(h);
            run_pw(h, L(h, P0 + ".b2.pw1"), cur, curC, 0, Mi, t1, bf, 0, nullptr, 0, 0);
            run_dw(h, L(h, P0 + ".b2.dw"), t1, bf, 0, B, curH, curW, t2, bf, 0);
            join_from(h, 0);
            run_pw(h, L(h, P0 + ".b2.pw2"), t2, bf, 0, Mo, oA, C, 0, tb1, bf, 0);     // cat + shuffle fused
        }
            }
        }
        float* o_cur = oA;
        float* o_nxt = oB;
        // stride-1 blocks (backbone/shufflenetv2.py:70-72; x1 = ch [0,bf) passes through, x2 = ch [bf,C)): one kernel per
        // unit, cut at the depthwise conv (unit_chain_kernel), after the first unit's pw1; else three kernels per unit
        const int R = STAGE_REP[si];
        const int chained = R > 1 ? (down_chained ? run_unit_chain(h, si + 2, R, o_cur, B, Ho, Wo, C, o_nxt, t2, t1, &o_cur, false, true)
                                                  : run_unit_chain(h, si + 2, R, o_cur, B, Ho, Wo, C, o_nxt, t1, t2, &o_cur)) : 0;
        if (down_chained && chained != 1) return fail(h, "stage %d: the chain the stride-2 unit prepared for did not run", si + 2);
        if (chained < 0) return 1;
        if (!chained) {
            for (int bi = 1; bi < R; ++bi) {
                snprintf(nm, sizeof nm, "backbone.stage%d.%d", si + 2, bi);
                const std::string P = nm;
                run_unit(h, P, o_cur, B, Ho, Wo, o_nxt, t1, t2);
                float* tmp = o_cur; o_cur = o_nxt; o_nxt = tmp;
            }
        }
        cfeat[si] = o_cur;
        if (h->tap_out[si]) HIPCHK(h, hipMemcpyAsync(h->tap_out[si], o_cur, (size_t)Mo * C * sizeof(float), hipMemcpyDeviceToDevice, h->cur));
        cur = o_cur; curC = C; curH = Ho; curW = Wo;
    }
    // neck: models/yolo_nano.py:286-296
    const int H3 = GH / 8, H4 = GH / 16, H5 = GH / 32, W3 = GW / 8, W4 = GW / 16, W5 = GW / 32;
    const long M3 = (long)B * H3 * W3, M4 = (long)B * H4 * W4, M5 = (long)B * H5 * W5;
    TAKE(p3, M3 * NECK); TAKE(p4, M4 * NECK); TAKE(p5, M5 * NECK);
    // the three laterals are independent (p3 is only needed by smooth_1): one grouped launch, or three launches with the large one
    // forked onto a side stream
    bool lat_grouped = false;
    if (h->group_launch && !exact(h)) {
        const Layer* ll[3] = {&L(h, "conv1x1_0"), &L(h, "conv1x1_1"), &L(h, "conv1x1_2")};
        if (ll[0]->ws_hi && ll[1]->ws_hi && ll[2]->ws_hi) {
            // longest K first: a workgroup of the K = 464 lateral runs 15 chunk rounds against 4 for the stride-8 one, and workgroups start
            // in id order - last in the grid, the few long ones were a 25 us tail behind the many short ones
            const Layer* lo[3] = {ll[2], ll[1], ll[0]};
            GemmArgs g3[3] = {pw_args(h, *ll[2], cfeat[2], h->stage_ch[2], 0, M5, p5, NECK, 0, nullptr, 0, 0),
                              pw_args(h, *ll[1], cfeat[1], h->stage_ch[1], 0, M4, p4, NECK, 0, nullptr, 0, 0),
                              pw_args(h, *ll[0], cfeat[0], h->stage_ch[0], 0, M3, p3, NECK, 0, nullptr, 0, 0)};
            lat_grouped = run_pw_group(h, lo, g3, 3, "conv1x1_*");
        }
    }
    if (!lat_grouped) {
        fork_to(h, 0);
        run_pw(h, L(h, "conv1x1_0"), cfeat[0], h->stage_ch[0], 0, M3, p3, NECK, 0, nullptr, 0, 0);
        back_to_main(h);
        run_pw(h, L(h, "conv1x1_1"), cfeat[1], h->stage_ch[1], 0, M4, p4, NECK, 0, nullptr, 0, 0);
        run_pw(h, L(h, "conv1x1_2"), cfeat[2], h->stage_ch[2], 0, M5, p5, NECK, 0, nullptr, 0, 0);
    }
    TAKE(p4a, M4 * NECK); TAKE(p3a, M3 * NECK); TAKE(p4b, M4 * NECK); TAKE(p5a, M5 * NECK);
    run_c3(h, L(h, "smooth_0"), p4, p5, 1, B, H4, W4, p4a);        // p4 + up2(p5)
    join_from(h, 0);
    run_c3(h, L(h, "smooth_1"), p3, p4a, 1, B, H3, W3, p3a);       // p3 + up2(p4)
    // heads: models/yolo_nano.py:299-301.  head k only needs its own pyramid level, so head 1 (the big one) starts on a
    // side stream as soon as smooth_1 is enqueued, head 2 after smooth_2, head 3 stays on the main stream.
    const float* feats[3] = {p3a, p4b, p5a};
    const int Hs[3] = {H3, H4, H5}, Ws[3] = {W3, W4, W5};
    const bool fuse_all = head_fuse_all(h, B, fuse_decode);
    if (fused) *fused = fuse_all;
    auto run_head = [&](int hd) {
        const long M = (long)B * Hs[hd] * Ws[hd];
        float* hA = arena_take(h, (size_t)M * NECK);
        float* hB = arena_take(h, (size_t)M * NECK);
        float* hC = arena_take(h, (size_t)M * NECK);
        if (!hA || !hB || !hC) return 1;
        snprintf(nm, sizeof nm, "head_det_%d", hd + 1);
        const std::string P = nm;
        run_dwpw(h, L(h, P + ".0"), L(h, P + ".1"), feats[hd], NECK, 0, B, Hs[hd], Ws[hd], hA, hB, NECK, 0, nullptr, 0, 0);
        const float* const src[3] = {hB, hB, hB};           // (only entry hd is read)
        float* const sA[3] = {hA, hA, hA};
        float* const sC[3] = {hC, hC, hC};
        return run_head_tail(h, hd, B, src, sA, sC, heads, head_ld, fuse_all);
    };
    // All three heads layer by layer, each layer ONE grouped launch (5 launches instead of 15): the stride-16 / 32 heads ride along with
    // the stride-8 one instead of paying ten launches of 7-20 us for a few microseconds of work.  Needs the split-f16 family.
    if (heads_groupable(h)) {
        const Layer* hl[2][3];
        for (int k = 0; k < 2; ++k)
            for (int hd = 0; hd < 3; ++hd) {
                snprintf(nm, sizeof nm, "head_det_%d.%d", hd + 1, k);
                hl[k][hd] = &L(h, nm);
            }
        run_c3(h, L(h, "smooth_2"), p4a, p3a, 2, B, H4, W4, p4b);      // p4 + down(p3)
        run_c3(h, L(h, "smooth_3"), p5, p4b, 2, B, H5, W5, p5a);       // p5 + down(p4)
        float *hA[3], *hB[3], *hC[3];
        for (int hd = 0; hd < 3; ++hd) {
            const size_t M = (size_t)B * Hs[hd] * Ws[hd];
            hA[hd] = arena_take(h, M * NECK); hB[hd] = arena_take(h, M * NECK); hC[hd] = arena_take(h, M * NECK);
            if (!hA[hd] || !hB[hd] || !hC[hd]) return fail(h, "activation arena exhausted (%zu bytes)", h->arena_bytes);
        }
        const bool ok = head_dwpw_layer(h, hl[0], hl[1], B, nullptr, feats, hB, "head_det_*.0+1") ||
                        (head_dw_layer(h, hl[0], B, nullptr, feats, hA, "head_det_*.0") && head_pw_layer(h, hl[1], B, hA, hB, NECK, 0, "head_det_*.1"));
        if (!ok) return fail(h, "grouped head launch: unsupported layer layout");
        if (run_head_tail(h, -1, B, hB, hA, hC, heads, head_ld, fuse_all)) return 1;
    } else {
    fork_to(h, 0);
    if (run_head(0)) return fail(h, "activation arena exhausted (%zu bytes)", h->arena_bytes);
    back_to_main(h);
    run_c3(h, L(h, "smooth_2"), p4a, p3a, 2, B, H4, W4, p4b);      // p4 + down(p3)
    fork_to(h, 1);
    if (run_head(1)) return fail(h, "activation arena exhausted (%zu bytes)", h->arena_bytes);
    back_to_main(h);
    run_c3(h, L(h, "smooth_3"), p5, p4b, 2, B, H5, W5, p5a);       // p5 + down(p4)
    if (run_head(2)) return fail(h, "activation arena exhausted (%zu bytes)", h->arena_bytes);
    join_from(h, 0);
    join_from(h, 1);
    }
#undef TAKE
    HIPCHK(h, hipGetLastError());
    return 0;
}

int check_ready(yn_handle* h, int B)
{
    if (!h->folded) return fail(h, "weights not prepared: call yn_fold_bn() after loading parameters");
    if (B <= 0) return fail(h, "batch must be positive (got %d)", B);
    return 0;
}

// run `body` directly, or captured into / replayed from a hipGraph keyed by `key`
template <class F>
int run_maybe_graph(yn_handle* h, const std::vector<uintptr_t>& key, F body)
{
    if (!h->use_graph || h->profiling) return body();
    if (h->stream == nullptr)                               // the legacy default stream cannot be captured; trying leaves the runtime in capture-error state
        return fail(h, "hipGraph capture needs a non-default stream: create the handle on (or yn_set_stream to) a stream of its own");
    for (GraphEntry& g : h->graphs)
        if (g.key == key) { HIPCHK(h, hipGraphLaunch(g.exec, h->stream)); return 0; }
    if (h->autotune) { const int rc0 = body(); if (rc0) return rc0; }      // eager pass: tunes tile configurations, warms up
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(h, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    GraphEntry ge;
    ge.key = key;
    HIPCHK(h, hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    h->graphs.push_back(ge);
    HIPCHK(h, hipGraphLaunch(ge.exec, h->stream));
    return 0;
}

}  // namespace

// =================================================================================================
#pragma GCC visibility push(default)
extern "C" {

int yn_abi_version(void) { return 2; }       // 2: + yn_range_status, yn_allreduce_grads, yn_tune_save / yn_tune_load, yn_train_get / set_loss_scale

const char* yn_last_error(yn_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int yn_live_device_memory(int64_t* blocks, int64_t* bytes)
{
    if (blocks) *blocks = g_live_blocks.load();
    if (bytes) *bytes = g_live_bytes.load();
    return 0;
}

int yn_create(const yn_config* cfg, yn_handle** out)
{
    if (!cfg || !out) return fail(nullptr, "yn_create: null argument");
    *out = nullptr;
    if (cfg->backbone < 0 || cfg->backbone > 3)
        return fail(nullptr, "unsupported backbone id %d (0.5x/1.0x/1.5x/2.0x = 0..3)", cfg->backbone);   // models/yolo_nano.py:35-37
    if (cfg->num_anchors < 1 || cfg->num_anchors > 3) return fail(nullptr, "num_anchors must be 1..3");
    if (cfg->num_classes < 1 || cfg->num_classes > 1024) return fail(nullptr, "num_classes out of range");
    if (cfg->input_size <= 0 || cfg->input_size % 32) return fail(nullptr, "input_size must be a positive multiple of 32");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, "no HIP device available (%s)", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "device %d out of range (%d devices)", cfg->device, ndev);
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(nullptr, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    yn_handle* h = new yn_handle();
    h->cfg = *cfg;
    if (h->cfg.max_batch < 1) h->cfg.max_batch = 1;
    h->stream = (hipStream_t)cfg->stream;
    h->cur = h->stream;
    h->nms.prefilter = 1;
    h->nms.sweep = 1;
    build_layers(h);
    if (set_grid_info(h, cfg->input_size)) { g_create_error = h->err; delete h; return 1; }
    // (hipMemsetAsync on the handle's stream, never hipMemset: ONE operation on the legacy null stream and every later launch of the
    // process on torch's streams serialises against it - measured 38.2 k -> 32.6 k images/s with four handles, single-stream unchanged)
    if (h->range_flags.reserve(3) ||
        hipMemsetAsync(h->range_flags, 0, 3 * sizeof(unsigned), h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
        g_create_error = "yn_create: out of device memory"; delete h; return 1;
    }
    if (h->range_host.reserve(1) ||      // coherent: the kernel's system-scope store is visible when it is made, not at kernel end (HIP_HOST_COHERENT=0)
        hipHostGetDevicePointer((void**)&h->range_host_dev, h->range_host.get(), 0) != hipSuccess) {
        g_create_error = "yn_create: no pinned host memory for the range flag"; delete h; return 1;
    }
    h->range_host[0] = 0;
    *out = h;
    return 0;
}

void yn_destroy(yn_handle* h)
{
    if (!h) return;
    DevGuard dev_guard_(h);
    (void)hipStreamSynchronize(h->stream);
    for (GraphEntry& g : h->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
    if (h->tune_e0) { (void)hipEventDestroy(h->tune_e0); (void)hipEventDestroy(h->tune_e1); }
    for (hipEvent_t e : h->fj_events) (void)hipEventDestroy(e);
    for (int k = 0; k < 2; ++k) if (h->side[k]) (void)hipStreamDestroy(h->side[k]);
    for (TrainGraph& g : h->train_graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (h->train_side) (void)hipStreamDestroy(h->train_side);
    for (int i = 0; i < 2; ++i) if (h->train_fork[i]) (void)hipStreamDestroy(h->train_fork[i]);
    for (int i = 0; i < 8; ++i) if (h->fork_ev[i]) (void)hipEventDestroy(h->fork_ev[i]);
    for (hipEvent_t e : h->train_events) (void)hipEventDestroy(e);
    delete h;                                // every buffer goes with its owning member, on the handle's device (dev_guard_)
}

int yn_set_grid(yn_handle* h, int input_size)
{
    YN_ENTER(h);
    if (set_grid_info(h, input_size)) return 1;
    h->cfg.input_size = input_size;
    return 0;
}

// A rectangular grid: the H x W window at (left, top) of a letterboxed side x side square (side = 0: the smallest square, the window centred).
// The window that is the whole square is yn_set_grid(side).
int yn_set_grid_rect(yn_handle* h, int height, int width, int side, int left, int top)
{
    YN_ENTER(h);
    if (height <= 0 || width <= 0 || (height % 32) != 0 || (width % 32) != 0)
        return fail(h, "yn_set_grid_rect: the extents %d x %d are not positive multiples of 32", height, width);
    if (side == 0) {
        side = height > width ? height : width;
        left = (side - width) / 2; top = (side - height) / 2;
    }
    if (side < 0 || left < 0 || top < 0 || (long)left + width > side || (long)top + height > side)
        return fail(h, "yn_set_grid_rect: the %d x %d window at (%d, %d) lies outside the %d x %d square", height, width, left, top, side, side);
    if (set_grid_window(h, height, width, side, left, top)) return 1;
    if (!h->grid.win) h->cfg.input_size = side;
    return 0;
}

int yn_grid_shape(yn_handle* h, int* height, int* width, int* side, int* left, int* top)
{
    YN_ENTER(h);
    const GridInfo& g = h->grid;
    if (height) *height = g.H;
    if (width) *width = g.W;
    if (side) *side = g.side;
    if (left) *left = g.left;
    if (top) *top = g.top;
    return 0;
}

int yn_set_stream(yn_handle* h, void* stream)
{
    YN_ENTER(h);
    if ((hipStream_t)stream != h->stream) {
        HIPCHK(h, hipStreamSynchronize(h->stream));        // the arena is shared: drain the old stream first
        drop_graphs(h);
    }
    h->stream = (hipStream_t)stream;
    h->cur = h->stream;
    return 0;
}

int yn_set_thresholds(yn_handle* h, float conf_thresh, float nms_thresh, int diou_nms)
{
    YN_ENTER(h);
    if (conf_thresh != h->cfg.conf_thresh || nms_thresh != h->cfg.nms_thresh || diou_nms != h->cfg.diou_nms) {
        drop_graphs(h);
    }
    h->cfg.conf_thresh = conf_thresh; h->cfg.nms_thresh = nms_thresh; h->cfg.diou_nms = diou_nms;
    return 0;
}

int yn_num_predictions(yn_handle* h) { return h ? h->grid.N : -1; }

int yn_use_graph(yn_handle* h, int enable) { if (!h) return 1; h->use_graph = enable != 0; return 0; }

int yn_autotune(yn_handle* h, int enable)
{
    YN_ENTER(h);
    h->autotune = enable != 0;                              // off: this handle uses the static heuristic; the shared table stays
    return 0;
}

int yn_set_pw_config(yn_handle* h, int index)
{
    YN_ENTER(h);
    if (index >= pw_config_count()) return fail(h, "yn_set_pw_config: index %d out of range (%d configurations)", index, pw_config_count());
    h->force_pw_cfg = index < 0 ? -1 : index;
    return 0;
}
// The autotuner's table (layer shape -> fastest tile configuration), shared by every handle of the process, to / from a text file:
// one line per entry, the device ordinal left out, so that the ranks of a multi-GPU job can adopt ONE rank's choices (identical
// GPUs, identical shapes: eight ranks timing the same ~40 shapes at once only adds noise to each other's brackets and lets replicas
// end up on different tiles).  Every configuration gives the same bits; this is a speed matter only.
int yn_tune_save(const char* path, int device)
{
    if (!path) return 1;
    FILE* f = fopen(path, "w");
    if (!f) return 1;
    std::lock_guard<std::mutex> lk(g_tune_mutex);
    for (const auto& kv : g_pw_tuned) {
        if (kv.first.empty() || kv.first[0] != device) continue;
        fprintf(f, "%d", kv.second);
        for (size_t i = 1; i < kv.first.size(); ++i) fprintf(f, " %d", kv.first[i]);
        fprintf(f, "\n");
    }
    fclose(f);
    return 0;
}

int yn_tune_load(const char* path, int device)
{
    if (!path) return -1;
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int n = 0;
    char line[1024];
    std::lock_guard<std::mutex> lk(g_tune_mutex);
    while (fgets(line, sizeof line, f)) {
        std::vector<int> v;
        char* p = line;
        for (;;) {
            char* e = nullptr;
            const long x = strtol(p, &e, 10);
            if (e == p) break;
            v.push_back((int)x);
            p = e;
        }
        if (v.size() < 2 || v[0] < 0 || v[0] >= pw_config_count()) continue;
        std::vector<int> key;
        key.push_back(device);
        key.insert(key.end(), v.begin() + 1, v.end());
        if (!g_pw_tuned.count(key)) { g_pw_tuned[key] = v[0]; ++n; }
    }
    fclose(f);
    return n;
}

int yn_pw_config_count(void) { return pw_config_count(); }
int yn_pw_f32_config_count(void) { return pw_f32_config_count(); }
int yn_nms_prefilter(yn_handle* h, int mode)
{
    YN_ENTER(h);
    if (mode < 0 || mode > 2) return fail(h, "yn_nms_prefilter: mode %d is not 0, 1 or 2", mode);
    if (mode != h->nms.prefilter) drop_graphs(h);
    h->nms.prefilter = mode;
    return 0;
}
int yn_nms_sweep_segments(yn_handle* h, int B, int C)
{
    YN_ENTER(h);
    if (!h->nms.seg_sparse || B <= 0 || C <= 0 || (size_t)B * C > h->nms_seg[7].cap()) return 0;
    std::vector<int32_t> v((size_t)B * C);
    if (hipMemcpyAsync(v.data(), h->nms.seg_sparse, v.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    int k = 0;
    for (int32_t x : v) k += x == 1;
    return k;
}
int yn_nms_stages(yn_handle* h, int B, int N, int C, int32_t* plan, int32_t* seg_count, int32_t* seg_off, int32_t* bucket, float* sbox,
                  int32_t* seg_count2, int32_t* bucket2, float* sbox2, int32_t* seg_sparse, int32_t* keep)
{
    YN_ENTER(h);
    const NmsPlan& p = h->nms_plan;
    if (B <= 0 || N <= 0 || C <= 0 || p.B != B || p.N != N || p.C != C)
        return fail(h, "yn_nms_stages: (B, N, C) = (%d, %d, %d), the last NMS call had (%d, %d, %d)", B, N, C, p.B, p.N, p.C);
    const size_t cand = (size_t)B * N, seg = (size_t)B * C;
    if (cand > h->nms_bucket.cap() || cand > h->nms_keep.cap() || cand * 4 > h->nms_sbox.cap() || cand > h->nms_bucket2.cap() || cand * 4 > h->nms_sbox2.cap() ||
        seg > h->nms_seg[0].cap() || !h->nms.seg_count)
        return fail(h, "yn_nms_stages: the handle holds no NMS scratch of that size");
    if (plan) {
        const int32_t v[YN_NMS_PLAN_INTS] = {p.B, p.N, p.C, p.few, p.fused, p.chunks, p.merge, p.prefilter, p.pre_ranks, p.sweep, p.sweep_maxn, p.sweep_slots,
                                             p.sweep_split, p.resolve_one, p.resolve_split, p.diou};
        for (int i = 0; i < YN_NMS_PLAN_INTS; ++i) plan[i] = v[i];
    }
    auto get = [&](void* dst, const void* src, size_t bytes) {
        if (dst) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
        return 0;
    };
    if (get(seg_count, h->nms.seg_count, seg * 4) || get(seg_off, h->nms.seg_off, seg * 4) || get(bucket, h->nms.bucket, cand * 4) ||
        get(sbox, h->nms.sbox, cand * 16) || get(keep, h->nms.keep, cand * 4)) return 1;
    if (p.prefilter && (get(seg_count2, h->nms.seg_count2, seg * 4) || get(bucket2, h->nms.bucket2, cand * 4) || get(sbox2, h->nms.sbox2, cand * 16) ||
                        get(seg_sparse, h->nms.seg_sparse, seg * 4))) return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
int yn_nms_sweep(yn_handle* h, int enable)
{
    if (!h) return 1;
    if ((enable != 0) != (h->nms.sweep != 0)) drop_graphs(h);
    h->nms.sweep = enable != 0;
    return 0;
}

int yn_down_fuse(yn_handle* h, int enable)
{
    YN_ENTER(h);
    if ((enable != 0) != h->down_fuse) drop_graphs(h);
    h->down_fuse = enable != 0;
    return 0;
}

int yn_tail_fuse(yn_handle* h, int enable)
{
    YN_ENTER(h);
    if ((enable != 0) != h->tail_fuse) drop_graphs(h);
    h->tail_fuse = enable != 0;
    return 0;
}

int yn_group_launch(yn_handle* h, int enable)
{
    YN_ENTER(h);
    if ((enable != 0) != h->group_launch) drop_graphs(h);
    h->group_launch = enable != 0;
    return 0;
}

int yn_fuse_decode(yn_handle* h, int enable)
{
    YN_ENTER(h);
    if ((enable != 0) != h->fuse_decode || enable != h->fuse_decode_mode) drop_graphs(h);
    h->fuse_decode = enable != 0;
    h->fuse_decode_mode = enable;
    return 0;
}

int yn_exact_f32(yn_handle* h, int enable)
{
    YN_ENTER(h);
    if ((enable != 0) != h->exact_f32) drop_graphs(h);
    h->exact_f32 = enable != 0;
    return 0;
}
int yn_multi_stream(yn_handle* h, int enable) { if (!h) return 1; h->multi_stream = enable != 0; return 0; }
int yn_unit_chain(yn_handle* h, int mode) { if (!h) return 1; h->unit_chain = mode < 0 ? 0 : (mode > 2 ? 2 : mode); return 0; }
int yn_chain_pipe(yn_handle* h, int mode)
{
    if (!h) return 1;
    const int m = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
    if (m != h->chain_pipe) drop_graphs(h);
    h->chain_pipe = m;
    return 0;
}
int yn_stage_fuse(yn_handle* h, int mode, int publish_early)
{
    if (!h) return 1;
    const int m = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
    if (m != h->stage_fuse || (publish_early != 0) != (h->stage_pub_early != 0)) drop_graphs(h);
    h->stage_fuse = m;
    h->stage_pub_early = publish_early != 0;
    return 0;
}
int yn_pw_pipe(yn_handle* h, int enable)
{
    if (!h) return 1;
    if ((enable != 0) != h->pw_pipe) drop_graphs(h);
    h->pw_pipe = enable != 0;
    return 0;
}

int yn_synchronize(yn_handle* h) { YN_ENTER(h); HIPCHK(h, hipStreamSynchronize(h->stream)); return 0; }

// ---- weights -----------------------------------------------------------------------------------
static int load_param_impl(yn_handle* h, const char* key, const void* ptr, const int64_t* shape, int ndim, bool from_dev)
{
    if (!h || !key) return 1;
    if (!ptr) return fail(h, "yn_load_param(%s): null data", key);
    const std::string k = key;
    const bool is_i64 = k.size() > 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0;
    if (is_i64) return 0;                                   // bookkeeping counter, unused in eval
    // validate the key against the architecture
    const size_t dot = k.rfind('.');
    if (dot == std::string::npos) return fail(h, "unknown state-dict key '%s'", key);
    const std::string prefix = k.substr(0, dot), leaf = k.substr(dot + 1);
    const Layer* owner = nullptr;
    bool is_bn = false;
    auto it = h->by_conv.find(prefix);
    if (it != h->by_conv.end() && (leaf == "weight" || leaf == "bias")) owner = &h->layers[it->second];
    if (!owner) {
        for (const Layer& l : h->layers)
            if (!l.bn.empty() && l.bn == prefix) { owner = &l; is_bn = true; break; }
    }
    if (!owner) return fail(h, "unexpected state-dict key '%s'", key);
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
    size_t expect;
    if (is_bn || leaf == "bias") expect = owner->cout;
    else if (owner->kind == K_DW) expect = (size_t)owner->cout * 9;
    else if (owner->kind == K_PW) expect = (size_t)owner->cout * owner->cin;
    else expect = (size_t)owner->cout * owner->cin * 9;
    if (numel != expect) return fail(h, "size mismatch for '%s': got %zu elements, expected %zu", key, numel, expect);
    Param& p = h->params[k];
    const size_t bytes = numel * sizeof(float);
    if (p.dev.cap() != numel) {
        if (p.dev) { HIPCHK(h, hipStreamSynchronize(h->stream)); p.dev.reset(); }
        HIPCHK(h, p.dev.reserve(numel));
    }
    p.numel = numel;
    p.shape.assign(shape, shape + ndim);
    HIPCHK(h, hipMemcpyAsync(p.dev, ptr, bytes, from_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!from_dev) HIPCHK(h, hipStreamSynchronize(h->stream));   // host buffer may be freed by the caller
    h->folded = false;
    return 0;
}

int yn_load_param(yn_handle* h, const char* key, const void* host_ptr, const int64_t* shape, int ndim)
{
    return load_param_impl(h, key, host_ptr, shape, ndim, false);
}

int yn_load_param_dev(yn_handle* h, const char* key, const void* dev_ptr, const int64_t* shape, int ndim)
{
    return load_param_impl(h, key, dev_ptr, shape, ndim, true);
}

int yn_fold_bn(yn_handle* h)
{
    YN_ENTER(h);
    if (h->tP)                                              // after training: the flat buffer holds the current parameters
        for (const auto& kv : h->toff) {
            const Param* p = find_param(h, kv.first);
            if (p) HIPCHK(h, hipMemcpyAsync(p->dev, h->tP + kv.second, p->numel * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        }
    HIPCHK(h, hipMemsetAsync(h->range_flags, 0, sizeof(unsigned), h->stream));
    for (Layer& l : h->layers) {
        const Param* w = find_param(h, l.conv + ".weight");
        if (!w) return fail(h, "missing parameter '%s.weight'", l.conv.c_str());
        const Param* b = find_param(h, l.conv + ".bias");
        const Param *g = nullptr, *be = nullptr, *mu = nullptr, *var = nullptr;
        if (!l.bn.empty()) {
            g = find_param(h, l.bn + ".weight"); be = find_param(h, l.bn + ".bias");
            mu = find_param(h, l.bn + ".running_mean"); var = find_param(h, l.bn + ".running_var");
            const int have = (g != nullptr) + (be != nullptr) + (mu != nullptr) + (var != nullptr);
            if (have != 0 && have != 4) return fail(h, "incomplete BatchNorm parameters for '%s'", l.bn.c_str());
            if (have == 0 && !b) return fail(h, "'%s' has neither BatchNorm statistics nor a folded bias", l.conv.c_str());
        } else if (!b) return fail(h, "missing parameter '%s.bias'", l.conv.c_str());
        FoldArgs a{};
        a.w = (const float*)w->dev; a.b = b ? (const float*)b->dev : nullptr;
        a.gamma = g ? (const float*)g->dev : nullptr; a.beta = be ? (const float*)be->dev : nullptr;
        a.mean = mu ? (const float*)mu->dev : nullptr; a.var = var ? (const float*)var->dev : nullptr;
        a.eps = 1e-5f;
        a.Cout = l.cout; a.Cin = l.cin;
        size_t packed_floats;
        if (l.kind == K_DW) { a.kind = 1; a.kk = 9; packed_floats = (size_t)9 * l.cout; l.Npad = l.cout; l.Kp = 9; }
        else if (l.kind == K_STEM) { a.kind = 2; a.kk = 9; packed_floats = (size_t)27 * l.cout; l.Npad = l.cout; l.Kp = 27; }
        else {
            a.kind = 0; a.kk = (l.kind == K_DENSE3) ? 9 : 1;
            const int K = l.cin * a.kk;
            l.Kp = (K + 1) & ~1; l.Npad = (l.cout + 31) & ~31;
            packed_floats = (size_t)l.Kp * l.Npad;
        }
        a.Kp = l.Kp; a.Npad = l.Npad;
        // (no-ops from the second fold on: a layer's sizes never change)
        HIPCHK(h, l.w_packed.reserve(packed_floats));
        HIPCHK(h, l.b_packed.reserve((size_t)((l.Npad + 31) & ~31)));
        HIPCHK(h, l.w_ref.reserve(w->numel));
        HIPCHK(h, l.b_ref.reserve((size_t)l.cout));
        l.w_numel = w->numel;
        if (l.kind == K_DENSE3 || l.kind == K_PW) {
            const size_t halves = (size_t)(l.kind == K_DENSE3 ? 9 : 1) * ((l.cin + 7) / 8) * l.Npad * 8;
            HIPCHK(h, l.ws_hi.reserve(halves));
            HIPCHK(h, l.ws_lo.reserve(halves));
            HIPCHK(h, hipMemsetAsync(l.ws_hi, 0, l.ws_bytes(), h->stream));
            HIPCHK(h, hipMemsetAsync(l.ws_lo, 0, l.ws_bytes(), h->stream));
        }
        a.ws_hi = l.ws_hi.get(); a.ws_lo = l.ws_lo.get(); a.w_ovf = h->range_flags;
        HIPCHK(h, hipMemsetAsync(l.w_packed, 0, packed_floats * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(l.b_packed, 0, (size_t)((l.Npad + 31) & ~31) * sizeof(float), h->stream));
        a.w_ref = l.w_ref; a.b_ref = l.b_ref; a.w_packed = l.w_packed; a.b_packed = l.b_packed;
        launch_fold_pack(a, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    // Range guard of the split-f16 family (yn_device.h): a folded weight w * gamma / sqrt(var + eps) that does not fit x = hi + lo * 2^-11
    // (|w| >= 65504) would make its hi part inf and every product NaN where the reference's fp32 conv is finite.  One flag, read once per
    // fold: the handle then runs the f32-MFMA family as under yn_exact_f32(1) (yn_range_status reports it).
    unsigned wflag = 0;
    HIPCHK(h, hipMemcpyAsync(&wflag, h->range_flags, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((wflag != 0) != h->range_fallback) drop_graphs(h);
    h->range_fallback = wflag != 0;
    h->folded = true;
    return 0;
}

// The out-of-band form of yn_infer's range mark: compact_kernel set the handle's pinned word, nobody has acknowledged it through
// yn_range_status yet.  No synchronisation: the word is host memory.
static int range_pending(yn_handle* h, const char* who)
{
    // (not under yn_exact_f32: the f32-MFMA family cannot raise the flag, and running again under it IS the documented recovery - ADVICE r5)
    if (!exact(h) && h->range_host && __atomic_load_n(h->range_host.get(), __ATOMIC_RELAXED)) {
        fail(h, "%s: an earlier yn_infer split an activation >= 65504 (split-f16 range): its results are invalid - call yn_range_status to acknowledge, "
                "then yn_exact_f32(h, 1) and run again", who);
        return YN_STATUS_RANGE;
    }
    return 0;
}

int yn_range_status(yn_handle* h, int* weights_exceed_f16, int* activation_overflow)
{
    YN_ENTER(h);
    unsigned f = 0;
    HIPCHK(h, hipMemcpyAsync(&f, h->range_flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (f) HIPCHK(h, hipMemsetAsync(h->range_flags + 1, 0, sizeof(unsigned), h->stream));
    if (h->range_host) __atomic_store_n(h->range_host.get(), 0u, __ATOMIC_RELAXED);      // acknowledged (the stream is idle: no compact_kernel can still set it)
    if (h->stage_sync) {                                                            // stage_pipe_kernel's bounded waits (kernels_stage.hip): an expired one marks the launch
        unsigned tmo = 0;
        HIPCHK(h, hipMemcpyAsync(&tmo, h->stage_sync + STAGE_TIMEOUT, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (tmo) {
            HIPCHK(h, hipMemsetAsync(h->stage_sync + STAGE_TIMEOUT, 0, sizeof(unsigned), h->stream));
            return fail(h, "stage_pipe_kernel: a bounded wait for a tile's ready flag expired (2 s): the results of that call are invalid; yn_stage_fuse(h, 0, 1) runs the units one launch each");
        }
    }
    if (weights_exceed_f16) *weights_exceed_f16 = h->range_fallback ? 1 : 0;
    if (activation_overflow) *activation_overflow = f ? 1 : 0;
    return 0;
}

int yn_get_folded(yn_handle* h, const char* conv_key, float* host_weight, float* host_bias)
{
    YN_ENTER(h);
    if (!h->folded) return fail(h, "yn_get_folded before yn_fold_bn");
    auto it = h->by_conv.find(conv_key);
    if (it == h->by_conv.end()) return fail(h, "unknown conv '%s'", conv_key);
    const Layer& l = h->layers[it->second];
    HIPCHK(h, hipMemcpyAsync(host_weight, l.w_ref, l.w_numel * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(host_bias, l.b_ref, (size_t)l.cout * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- network -----------------------------------------------------------------------------------
int yn_forward_raw(yn_handle* h, const float* x_dev, int B, float* head_s8, float* head_s16, float* head_s32)
{
    YN_ENTER(h);
    if (check_ready(h, B)) return 1;
    const GridInfo& g = h->grid;
    if (ensure_arena(h, B, g.H, g.W)) return 1;
    float* const heads[3] = {head_s8, head_s16, head_s32};
    // (the window is part of the key: a captured graph holds the grid it was captured with, GridInfo travels by value in the kernel arguments)
    std::vector<uintptr_t> key = {1, (uintptr_t)B, (uintptr_t)g.H, (uintptr_t)g.W, (uintptr_t)g.side, (uintptr_t)g.left, (uintptr_t)g.top, (uintptr_t)x_dev,
                                  (uintptr_t)head_s8, (uintptr_t)head_s16, (uintptr_t)head_s32};
    return run_maybe_graph(h, key, [&]() { return run_network(h, x_dev, B, heads, h->head_ch); });
}

int yn_forward_taps(yn_handle* h, const float* x_dev, int B, float* c3_dev, float* c4_dev, float* c5_dev)
{
    YN_ENTER(h);
    if (check_ready(h, B)) return 1;
    if (!c3_dev || !c4_dev || !c5_dev) return fail(h, "yn_forward_taps: null output");
    if (ensure_arena(h, B, h->grid.H, h->grid.W) || ensure_heads(h, B)) return 1;
    float* const heads[3] = {h->heads_int[0], h->heads_int[1], h->heads_int[2]};
    h->tap_out[0] = c3_dev; h->tap_out[1] = c4_dev; h->tap_out[2] = c5_dev;
    const int rc = run_network(h, x_dev, B, heads, (h->head_ch + 3) & ~3);       // eager: the taps are not part of any captured graph
    h->tap_out[0] = h->tap_out[1] = h->tap_out[2] = nullptr;
    return rc;
}

int yn_score_full(yn_handle* h, const float* h8, const float* h16, const float* h32, int B, float* all_bbox, float* all_class)
{
    YN_ENTER(h);
    const float* const heads[3] = {h8, h16, h32};
    h->cur = h->stream;
    {
        Bracket br(h, "score_full", 0.0, 0.0);
        launch_score_full(heads, h->grid, B, all_bbox, all_class, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_decode_boxes(yn_handle* h, const float* txtytwth, int B, float* xyxy)
{
    YN_ENTER(h);
    launch_decode_boxes(txtytwth, h->grid, B, xyxy, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_create_grid(yn_handle* h, int input_size, float* grid, float* stride, float* anchor)
{
    YN_ENTER(h);
    if (input_size <= 0 || input_size % 32) return fail(h, "input_size must be a positive multiple of 32");
    return yn_create_grid_rect(h, input_size, input_size, grid, stride, anchor);
}

int yn_create_grid_rect(yn_handle* h, int height, int width, float* grid, float* stride, float* anchor)
{
    YN_ENTER(h);
    if (height <= 0 || width <= 0 || height % 32 || width % 32) return fail(h, "yn_create_grid_rect: the extents %d x %d are not positive multiples of 32", height, width);
    const int A = h->cfg.num_anchors;
    size_t cell = 0;
    for (int s = 0; s < 3; ++s) {
        const int st = 8 << s, w = width / st, hh = height / st;
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < w; ++x, ++cell) {
                grid[cell * 2 + 0] = (float)x; grid[cell * 2 + 1] = (float)y;      // (x, y): models/yolo_nano.py:96
                for (int a = 0; a < A; ++a) {
                    stride[(cell * A + a) * 2 + 0] = (float)st; stride[(cell * A + a) * 2 + 1] = (float)st;
                    anchor[(cell * A + a) * 2 + 0] = h->cfg.anchors[(s * A + a) * 2 + 0];
                    anchor[(cell * A + a) * 2 + 1] = h->cfg.anchors[(s * A + a) * 2 + 1];
                }
            }
    }
    return 0;
}

// ---- post-processing ---------------------------------------------------------------------------
int yn_nms(yn_handle* h, const float* dets, const float* scores, int n, float nms_thresh, int diou, int32_t* keep, int32_t* count)
{
    YN_ENTER(h);
    if (n < 0) return fail(h, "yn_nms: negative n");
    if (ensure_post(h, 1, n > 0 ? n : 1, 1)) return 1;
    launch_nms_single(dets, scores, n, nms_thresh, diou, h->nms.bucket, h->nms.sbox, h->nms.matrix, keep, count, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_postprocess(yn_handle* h, const float* all_local, const float* all_conf, int B, int N, int C,
                   float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index, int32_t* count)
{
    YN_ENTER(h);
    if (B <= 0 || N < 0 || C <= 0) return fail(h, "yn_postprocess: bad sizes B=%d N=%d C=%d", B, N, C);
    if (N == 0) { HIPCHK(h, hipMemsetAsync(count, 0, sizeof(int32_t) * B, h->stream)); return 0; }
    const bool soft = h->soft_method != YN_SOFT_OFF;
    if (soft && h->cfg.diou_nms) return fail(h, "yn_postprocess: Soft-NMS (yn_soft_nms method %d) has no DIoU form; clear diou_nms or set YN_SOFT_OFF", h->soft_method);
    if (soft ? ensure_soft(h, B, N, C) : ensure_post(h, B, N, C)) return 1;
    launch_argmax_cand(all_local, all_conf, B, N, C, h->cfg.conf_thresh, h->cand_boxes, h->cand_scores, h->cand_cls, h->stream);
    if (soft)
        launch_soft_pipeline(h->cand_boxes, h->cand_scores, h->cand_cls, B, N, C, h->soft_method, h->cfg.nms_thresh, h->soft_sigma, h->soft_floor, h->nms,
                             h->soft, out_boxes, out_scores, out_cls, out_index, count, h->stream);
    else
        launch_nms_pipeline(h->cand_boxes, h->cand_scores, h->cand_cls, B, N, C, h->cfg.nms_thresh, h->cfg.diou_nms, h->nms,
                            out_boxes, out_scores, out_cls, out_index, count, h->stream, nullptr, &h->nms_plan);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_preprocess(yn_handle* h, const uint8_t* img, int h0, int w0, int rw, int rh, int left, int top, int side,
                  const float* mean, const float* stdv, float* x)
{
    YN_ENTER(h);
    if (!img || !x || !mean || !stdv) return fail(h, "yn_preprocess: null pointer");
    if (h0 <= 0 || w0 <= 0 || rw <= 0 || rh <= 0 || side <= 0 || left < 0 || top < 0 || left + rw > side || top + rh > side)
        return fail(h, "yn_preprocess: bad geometry (%dx%d -> %dx%d at (%d,%d) in %d)", w0, h0, rw, rh, left, top, side);
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_preprocess: std must be positive");
    launch_preprocess(img, h0, w0, rw, rh, left, top, side, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_preprocess_batch(yn_handle* h, int n, const uint8_t* const* imgs, const int32_t* geom, int side, const float* mean, const float* stdv, float* x)
{
    YN_ENTER(h);
    if (n == 0) return 0;                                   // an empty batch is not an error
    if (n < 0 || !imgs || !geom || !x || !mean || !stdv || side <= 0) return fail(h, "yn_preprocess_batch: bad arguments");
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_preprocess_batch: std must be positive");
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geom + (size_t)i * 6;
        if (!imgs[i] || g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0 || g[4] < 0 || g[5] < 0 || g[4] + g[2] > side || g[5] + g[3] > side)
            return fail(h, "yn_preprocess_batch: bad geometry for image %d", i);
    }
    launch_preprocess_batch(n, imgs, geom, side, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The win_w x win_h window at (win_left, win_top) of the tensor yn_preprocess_batch writes for the same images: x [n][3][win_h][win_w].
// A window that cuts into an image's resized extent is refused (the picture must survive whole; only pad is cut off).
int yn_preprocess_batch_rect(yn_handle* h, int n, const uint8_t* const* imgs, const int32_t* geom, int side, int win_left, int win_top, int win_w, int win_h,
                             const float* mean, const float* stdv, float* x)
{
    YN_ENTER(h);
    if (n == 0) return 0;
    if (n < 0 || !imgs || !geom || !x || !mean || !stdv || side <= 0) return fail(h, "yn_preprocess_batch_rect: bad arguments");
    if (win_w <= 0 || win_h <= 0 || win_left < 0 || win_top < 0 || (long)win_left + win_w > side || (long)win_top + win_h > side)
        return fail(h, "yn_preprocess_batch_rect: the %d x %d window at (%d, %d) lies outside the %d x %d square", win_h, win_w, win_left, win_top, side, side);
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_preprocess_batch_rect: std must be positive");
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geom + (size_t)i * 6;
        if (!imgs[i] || g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0 || g[4] < 0 || g[5] < 0 || g[4] + g[2] > side || g[5] + g[3] > side)
            return fail(h, "yn_preprocess_batch_rect: bad geometry for image %d", i);
        if (g[4] < win_left || g[5] < win_top || g[4] + g[2] > win_left + win_w || g[5] + g[3] > win_top + win_h)
            return fail(h, "yn_preprocess_batch_rect: the window [%d, %d) x [%d, %d) cuts image %d, whose resized extent is [%d, %d) x [%d, %d)", win_left,
                        win_left + win_w, win_top, win_top + win_h, i, g[4], g[4] + g[2], g[5], g[5] + g[3]);
    }
    launch_preprocess_batch_rect(n, imgs, geom, win_left, win_top, win_w, win_h, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

static_assert(YN_AUG_BRIGHTNESS == ynk::AUG_BRIGHT && YN_AUG_CONTRAST == ynk::AUG_CONTRAST && YN_AUG_CONTRAST_FIRST == ynk::AUG_CONTRAST_FIRST &&
              YN_AUG_SATURATION == ynk::AUG_SAT && YN_AUG_HUE == ynk::AUG_HUE, "yn_train_transform_batch flag bits");

int yn_train_transform_batch(yn_handle* h, int n, const uint8_t* const* imgs, const int32_t* geom, const float* photo, int side,
                             const float* mean, const float* stdv, float* x)
{
    YN_ENTER(h);
    if (n == 0) return 0;                                   // an empty batch is not an error
    if (n < 0 || side <= 0) return fail(h, "yn_train_transform_batch: bad arguments (n %d, side %d)", n, side);
    if (!imgs || !geom || !photo || !x || !mean || !stdv) return fail(h, "yn_train_transform_batch: null pointer");
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_train_transform_batch: std must be positive");
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geom + (size_t)i * ynk::AUG_GEOM;
        if (!imgs[i]) return fail(h, "yn_train_transform_batch: null frame pointer for image %d", i);
        if (g[0] <= 0 || g[1] <= 0 || g[2] < 0 || g[3] < 0 || g[4] <= 0 || g[5] <= 0 || g[4] > g[1] - g[2] || g[5] > g[0] - g[3])
            return fail(h, "yn_train_transform_batch: crop (%d,%d) %dx%d outside the %dx%d frame of image %d", g[2], g[3], g[4], g[5], g[1], g[0], i);
        if (g[7] <= 0 || g[8] <= 0 || g[9] < 0 || g[10] < 0 || g[7] > side - g[9] || g[8] > side - g[10])
            return fail(h, "yn_train_transform_batch: resized extent %dx%d at (%d,%d) outside %d for image %d", g[7], g[8], g[9], g[10], side, i);
        if ((g[6] != 0 && g[6] != 1) || (g[11] & ~ynk::AUG_FLAGS_ALL))
            return fail(h, "yn_train_transform_batch: bad mirror / flags (%d, %d) for image %d", g[6], g[11], i);
    }
    launch_train_aug_batch(n, imgs, geom, photo, side, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_mosaic_transform_batch(yn_handle* h, int n, const uint8_t* const* imgs, const int32_t* geom, const float* photo, int mosaic_size,
                              int side, const float* mean, const float* stdv, float* x)
{
    YN_ENTER(h);
    if (n == 0) return 0;                                   // an empty batch is not an error
    if (n < 0 || side <= 0 || mosaic_size <= 0 || mosaic_size > (1 << 14))
        return fail(h, "yn_mosaic_transform_batch: bad arguments (n %d, mosaic_size %d, side %d)", n, mosaic_size, side);
    if (!imgs || !geom || !photo || !x || !mean || !stdv) return fail(h, "yn_mosaic_transform_batch: null pointer");
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_mosaic_transform_batch: std must be positive");
    const int m2 = 2 * mosaic_size;
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geom + (size_t)i * ynk::MOS_GEOM;
        for (int k = 0; k < 4; ++k) {
            const int32_t* q = g + 12 * k;
            if (!imgs[(size_t)i * 4 + k]) return fail(h, "yn_mosaic_transform_batch: null frame pointer for mosaic %d frame %d", i, k);
            if (q[0] <= 0 || q[1] <= 0 || q[2] <= 0 || q[3] <= 0)
                return fail(h, "yn_mosaic_transform_batch: non-positive extent (%dx%d -> %dx%d) for mosaic %d frame %d", q[1], q[0], q[2], q[3], i, k);
            if (q[4] < 0 || q[5] < 0 || q[6] < q[4] || q[7] < q[5] || q[6] > m2 || q[7] > m2)
                return fail(h, "yn_mosaic_transform_batch: canvas rectangle (%d,%d)-(%d,%d) outside [0, %d] for mosaic %d frame %d", q[4], q[5], q[6], q[7], m2, i, k);
            if (q[8] < 0 || q[9] < 0 || q[10] < q[8] || q[11] < q[9] || q[10] > q[2] || q[11] > q[3])
                return fail(h, "yn_mosaic_transform_batch: source rectangle (%d,%d)-(%d,%d) outside the %dx%d resized frame for mosaic %d frame %d",
                            q[8], q[9], q[10], q[11], q[2], q[3], i, k);
            if (q[6] - q[4] != q[10] - q[8] || q[7] - q[5] != q[11] - q[9])
                return fail(h, "yn_mosaic_transform_batch: rectangle sizes differ (%dx%d canvas, %dx%d source) for mosaic %d frame %d",
                            q[6] - q[4], q[7] - q[5], q[10] - q[8], q[11] - q[9], i, k);
        }
        if ((g[48] != 0 && g[48] != 1) || (g[49] & ~ynk::AUG_FLAGS_ALL))
            return fail(h, "yn_mosaic_transform_batch: bad mirror / flags (%d, %d) for mosaic %d", g[48], g[49], i);
    }
    launch_mosaic_aug_batch(n, imgs, geom, photo, mosaic_size, side, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_nms_merge(yn_handle* h, const float* boxes, const float* scores, const int32_t* cls, int n, int num_classes, float nms_thresh, int diou,
                 float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index, int32_t* count)
{
    YN_ENTER(h);
    if (n < 0 || num_classes <= 0 || !count) return fail(h, "yn_nms_merge: bad arguments");
    if (n == 0) { HIPCHK(h, hipMemsetAsync(count, 0, sizeof(int32_t), h->stream)); return 0; }
    if (ensure_post(h, 1, n, num_classes)) return 1;
    launch_nms_pipeline(boxes, scores, cls, 1, n, num_classes, nms_thresh, diou, h->nms, out_boxes, out_scores, out_cls, out_index, count, h->stream, nullptr, &h->nms_plan);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_wbf_lds_clusters(void) { return ynk::YN_WBF_LDS_CLUSTERS; }
int64_t yn_wbf_cost(int64_t n_rows, int64_t n_clusters) { return (int64_t)ynk::wbf_cost(n_rows, n_clusters); }

int yn_wbf_merge(yn_handle* h, const float* boxes, const float* scores, const int32_t* cls, int n, int num_classes, float iou_thresh, int expected,
                 float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index, int32_t* out_votes, int32_t* assign, int32_t* count)
{
    YN_ENTER(h);
    if (!count) return fail(h, "yn_wbf_merge: count_dev is null");
    if (n < 0) return fail(h, "yn_wbf_merge: n is %d (a list has 0 or more rows)", n);
    if (expected < 1) return fail(h, "yn_wbf_merge: expected is %d (the expected votes are an integer of at least 1)", expected);
    if (num_classes != h->cfg.num_classes) return fail(h, "yn_wbf_merge: num_classes is %d, the handle has %d", num_classes, h->cfg.num_classes);
    if (n == 0) { HIPCHK(h, hipMemsetAsync(count, 0, sizeof(int32_t), h->stream)); return 0; }
    if (!boxes || !scores || !cls || !out_boxes || !out_scores || !out_cls) return fail(h, "yn_wbf_merge: null argument");
    if (ensure_wbf(h, 1, n, num_classes)) return 1;
    NmsWork wk = h->nms;
    wk.ovf = nullptr; wk.ovf_host = nullptr;
    launch_wbf_pipeline(boxes, scores, cls, 1, n, num_classes, iou_thresh, expected, wk, h->wbf, out_boxes, out_scores, out_cls, out_index, out_votes, assign,
                        count, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_soft_lds_rows(void) { return ynk::YN_SOFT_LDS_ROWS; }

int yn_soft_nms_merge(yn_handle* h, const float* boxes, const float* scores, const int32_t* cls, int n, int num_classes, int method, float iou_thresh,
                      float sigma, float score_floor, float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index, int32_t* count)
{
    YN_ENTER(h);
    if (!count) return fail(h, "yn_soft_nms_merge: count_dev is null");
    if (n < 0) return fail(h, "yn_soft_nms_merge: n is %d (a list has 0 or more rows)", n);
    if (soft_params(h, "yn_soft_nms_merge", YN_SOFT_HARD, method, sigma, score_floor)) return 1;
    if (num_classes != h->cfg.num_classes) return fail(h, "yn_soft_nms_merge: num_classes is %d, the handle has %d", num_classes, h->cfg.num_classes);
    if (n == 0) { HIPCHK(h, hipMemsetAsync(count, 0, sizeof(int32_t), h->stream)); return 0; }
    if (!boxes || !scores || !cls || !out_boxes || !out_scores || !out_cls) return fail(h, "yn_soft_nms_merge: null argument");
    if (ensure_soft(h, 1, n, num_classes)) return 1;
    NmsWork wk = h->nms;
    wk.ovf = nullptr; wk.ovf_host = nullptr;
    launch_soft_pipeline(boxes, scores, cls, 1, n, num_classes, method, iou_thresh, sigma, score_floor, wk, h->soft, out_boxes, out_scores, out_cls, out_index,
                         count, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_soft_nms(yn_handle* h, int method, float sigma, float score_floor)
{
    YN_ENTER(h);
    if (soft_params(h, "yn_soft_nms", YN_SOFT_OFF, method, sigma, score_floor)) return 1;
    if (method != h->soft_method || sigma != h->soft_sigma || score_floor != h->soft_floor) drop_graphs(h);
    h->soft_method = method; h->soft_sigma = sigma; h->soft_floor = score_floor;
    return 0;
}

int yn_op_soft_exp(yn_handle* h, const float* x, float* y, int64_t n)
{
    YN_ENTER(h);
    if (n < 0) return fail(h, "yn_op_soft_exp: n is %lld", (long long)n);
    if (n > 0 && (!x || !y)) return fail(h, "yn_op_soft_exp: null argument");
    launch_soft_exp(x, y, (long)n, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the candidate decode of raw heads that a forward wrote out (no fused front end ran): heads with row stride g.head_ld -> h->cand_*
static void decode_raw_heads(yn_handle* h, float* const heads[3], const GridInfo& g, int B)
{
    const float* const ch[3] = {heads[0], heads[1], heads[2]};
    Bracket br(h, "decode", 0.0, 4.0 * B * ((double)(g.N / g.A) * h->head_ch + 6.0 * g.N));
    launch_decode_cand(ch, g, B, h->cfg.conf_thresh, h->cand_boxes, h->cand_scores, h->cand_cls, h->stream);
}

int yn_infer(yn_handle* h, const float* x_dev, int B, float* out_boxes, float* out_scores, int32_t* out_cls,
             int32_t* out_index, int32_t* count)
{
    YN_ENTER(h);
    if (check_ready(h, B)) return 1;
    if (int rp = range_pending(h, "yn_infer")) return rp;
    GridInfo g = h->grid;
    g.head_ld = (h->head_ch + 3) & ~3;
    const bool soft = h->soft_method != YN_SOFT_OFF;
    if (soft && h->cfg.diou_nms) return fail(h, "yn_infer: Soft-NMS (yn_soft_nms method %d) has no DIoU form; clear diou_nms or set YN_SOFT_OFF", h->soft_method);
    if (ensure_arena(h, B, g.H, g.W) || (soft ? ensure_soft(h, B, g.N, g.C) : ensure_post(h, B, g.N, g.C)) || ensure_heads(h, B)) return 1;
    std::vector<uintptr_t> key = {2, (uintptr_t)B, (uintptr_t)g.H, (uintptr_t)g.W, (uintptr_t)g.side, (uintptr_t)g.left, (uintptr_t)g.top, (uintptr_t)x_dev, (uintptr_t)out_boxes, (uintptr_t)out_scores,
                                  (uintptr_t)out_cls, (uintptr_t)out_index, (uintptr_t)count};
    return run_maybe_graph(h, key, [&]() {
        float* const heads[3] = {h->heads_int[0], h->heads_int[1], h->heads_int[2]};
        bool fused = false;
        if (run_network(h, x_dev, B, heads, g.head_ld, true, &fused)) return 1;
        if (!fused) decode_raw_heads(h, heads, g, B);
        {
            // one profiling bracket per NMS kernel (the hook closes the previous one); bytes: candidate arrays read / written once
            struct Ctx { yn_handle* h; Bracket* cur; double bytes; } ctx{h, nullptr, 4.0 * B * 12.0 * g.N / 5.0};
            NmsHook hook{[](void* c, const char* k) {
                Ctx* x = (Ctx*)c;
                delete x->cur;
                set_last_kernel_name(k);
                x->cur = new Bracket(x->h, std::string("nms.") + k, 0.0, x->bytes);
            }, &ctx};
            NmsWork wk = h->nms;
            wk.ovf = exact(h) ? nullptr : h->range_flags + 1;         // the network's range flag rides out with the counts (compact_kernel)
            wk.ovf_host = exact(h) ? nullptr : h->range_host_dev;     // ... and into the handle's pinned word (range_pending)
            if (soft)
                launch_soft_pipeline(h->cand_boxes, h->cand_scores, h->cand_cls, B, g.N, g.C, h->soft_method, h->cfg.nms_thresh, h->soft_sigma, h->soft_floor,
                                     wk, h->soft, out_boxes, out_scores, out_cls, out_index, count, h->stream, h->profiling ? &hook : nullptr);
            else
                launch_nms_pipeline(h->cand_boxes, h->cand_scores, h->cand_cls, B, g.N, g.C, h->cfg.nms_thresh, h->cfg.diou_nms, wk,
                                    out_boxes, out_scores, out_cls, out_index, count, h->stream, h->profiling ? &hook : nullptr, &h->nms_plan);
            delete ctx.cur;
        }
        HIPCHK(h, hipGetLastError());
        return 0;
    });
}

int yn_pack_detections(yn_handle* h, const float* out_boxes, const float* out_scores, const int32_t* out_cls, const int32_t* count,
                       int B, int N, float* rec_dev, int32_t* offsets_dev)
{
    YN_ENTER(h);
    if (B <= 0 || N <= 0 || !out_boxes || !out_scores || !out_cls || !count || !rec_dev || !offsets_dev)
        return fail(h, "yn_pack_detections: bad arguments");
    if (int rp = range_pending(h, "yn_pack_detections")) return rp;
    launch_pack(out_boxes, out_scores, out_cls, count, B, N, rec_dev, offsets_dev, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- training loss ----------------------------------------------------------
static int ensure_loss(yn_handle* h, int B)
{
    const size_t need = (size_t)loss_num_blocks(h->grid, B) * 4;
    if (need <= h->loss_partial.cap()) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_train_graphs(h);                                   // a captured fp16 step carries loss_partial's address (launch_loss_h16)
    HIPCHK(h, h->loss_partial.reserve(need));
    return 0;
}

int yn_loss(yn_handle* h, const float* conf, const float* cls, const float* txtytwth, const float* target, int B,
            float* losses, float* g_conf, float* g_cls, float* g_txtytwth)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_loss")) return 1;
    if (B <= 0) return fail(h, "yn_loss: batch must be positive");
    if ((g_conf != nullptr) != (g_cls != nullptr) || (g_conf != nullptr) != (g_txtytwth != nullptr))
        return fail(h, "yn_loss: pass all three gradient buffers or none");
    if (ensure_loss(h, B)) return 1;
    if (g_cls) HIPCHK(h, hipMemsetAsync(g_cls, 0, (size_t)B * h->grid.N * h->grid.C * sizeof(float), h->stream));   // the kernel only writes the positives' class gradients
    launch_loss(conf, cls, txtytwth, nullptr, nullptr, target, h->grid, B, h->loss_partial, losses, g_conf, g_cls, g_txtytwth, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_loss_heads(yn_handle* h, const float* head_s8, const float* head_s16, const float* head_s32, const float* target, int B,
                  float* losses, float* g_s8, float* g_s16, float* g_s32)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_loss_heads")) return 1;
    if (B <= 0) return fail(h, "yn_loss_heads: batch must be positive");
    if ((g_s8 != nullptr) != (g_s16 != nullptr) || (g_s8 != nullptr) != (g_s32 != nullptr))
        return fail(h, "yn_loss_heads: pass all three gradient buffers or none");
    if (ensure_loss(h, B)) return 1;
    const float* const head[3] = {head_s8, head_s16, head_s32};
    float* const ghead[3] = {g_s8, g_s16, g_s32};
    if (g_s8)                                                   // the kernel only writes the positives' class gradients
        for (int k = 0; k < 3; ++k) HIPCHK(h, hipMemsetAsync(ghead[k], 0, (size_t)B * h->grid.hw[k] * h->grid.head_ld * sizeof(float), h->stream));
    launch_loss(nullptr, nullptr, nullptr, head, ghead, target, h->grid, B, h->loss_partial, losses, nullptr, nullptr, nullptr, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_make_targets(yn_handle* h, const double* labels_dev, const int32_t* offsets_dev, int B, const double* anchors_host, float* target_dev)
{
    YN_ENTER(h);
    if (need_square_grid(h, "yn_make_targets")) return 1;
    if (B <= 0 || !offsets_dev || !target_dev || !anchors_host) return fail(h, "yn_make_targets: bad arguments");
    if (h->grid.A != 3) return fail(h, "yn_make_targets: the label assigner is defined for 3 anchors per scale (got %d)", h->grid.A);
    HIPCHK(h, hipMemsetAsync(target_dev, 0, (size_t)B * h->grid.N * 11 * sizeof(float), h->stream));
    launch_make_targets(labels_dev, offsets_dev, B, anchors_host, h->grid, target_dev, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_ema_update(yn_handle* h, float* ema_dev, const float* model_dev, int64_t n, double decay)
{
    YN_ENTER(h);
    if (n < 0 || (n > 0 && (!ema_dev || !model_dev))) return fail(h, "yn_ema_update: bad arguments");
    if (n == 0) return 0;
    launch_ema(ema_dev, model_dev, (long)n, (float)decay, (float)(1.0 - decay), h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_sgd_step(yn_handle* h, float* params, const float* grads, float* momentum_buf, int64_t n,
                float lr, float momentum, float weight_decay, float grad_scale, int first_step)
{
    YN_ENTER(h);
    if (n < 0 || (n > 0 && (!params || !grads || !momentum_buf))) return fail(h, "yn_sgd_step: bad arguments");
    if (n == 0) return 0;                                   // an empty bucket: nothing to scan, nothing to step
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) return fail(h, "yn_sgd_step: buffers must be 16-byte aligned");
    if (!h->skip_flag) {
        HIPCHK(h, h->skip_flag.reserve(2));
        HIPCHK(h, hipMemsetAsync(h->skip_flag, 0, 2 * sizeof(int), h->stream));
    }
    launch_sgd(params, grads, momentum_buf, (long)n, lr, momentum, weight_decay, grad_scale, first_step, h->skip_flag, h->stream);
    // the fp16 step's loss scale follows the finite-scan of THIS bucket (after a data-parallel all-reduce: the same decision on every rank)
    if (h->scale_state && grads == h->tG) launch_hscale_update(h->scale_state, h->skip_flag, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_train_get_loss_scale(yn_handle* h, float* scale, float* clean_steps)
{
    YN_ENTER(h);
    float v[3] = {h->loss_scale_init >= 1.0f ? h->loss_scale_init : 1024.0f, 0.0f, h->loss_scale_clean};
    if (h->scale_state) {
        HIPCHK(h, hipMemcpyAsync(v, h->scale_state, sizeof v, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (scale) *scale = v[0];
    if (clean_steps) *clean_steps = v[2];
    return 0;
}

int yn_train_set_loss_scale(yn_handle* h, float scale, float clean_steps)
{
    YN_ENTER(h);
    // hscale_update_kernel halves down to 1 and doubles up to 65536; a larger restored value (up to 2^30: the overflow tests start there)
    // is accepted and can only shrink from then on
    if (!(scale >= 1.0f) || !(scale <= 1073741824.0f) || !(clean_steps >= 0.0f)) return fail(h, "yn_train_set_loss_scale: scale must lie in [1, 2^30], clean_steps >= 0");
    h->loss_scale_init = scale; h->loss_scale_clean = clean_steps;
    if (h->scale_state) {
        // all five words: a restored scale must not inherit the overflow flag / pending mark of an unsettled do_update = 0 step
        const float v[5] = {scale, 1.0f / scale, clean_steps, 0.0f, 0.0f};
        HIPCHK(h, hipMemcpyAsync(h->scale_state, v, sizeof v, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

// ---- single operators ----------------------------------------------------------------------------
namespace {
struct TmpLayer {
    Layer l;
    yn_handle* h;
    int rc = 0;
    TmpLayer(yn_handle* h_, int kind, int cin, int cout, int stride, int act, const float* w, const float* bias) : h(h_)
    {
        h->cur = h->stream;
        l.name = "op"; l.kind = kind; l.cin = cin; l.cout = cout; l.stride = stride; l.act = act;
        FoldArgs a{};
        a.w = w; a.b = bias; a.eps = 1e-5f; a.Cout = cout; a.Cin = cin;
        size_t packed;
        if (kind == K_DW) { a.kind = 1; a.kk = 9; packed = (size_t)9 * cout; l.Npad = cout; l.Kp = 9; }
        else if (kind == K_STEM) { a.kind = 2; a.kk = 9; packed = (size_t)27 * cout; l.Npad = cout; l.Kp = 27; }
        else { a.kind = 0; a.kk = kind == K_DENSE3 ? 9 : 1; const int K = cin * a.kk; l.Kp = (K + 1) & ~1; l.Npad = (cout + 31) & ~31; packed = (size_t)l.Kp * l.Npad; }
        a.Kp = l.Kp; a.Npad = l.Npad;
        const size_t bfl = (size_t)((l.Npad + 31) & ~31);
        if (l.w_packed.reserve(packed) || l.b_packed.reserve(bfl)) { rc = 1; return; }
        (void)hipMemsetAsync(l.w_packed, 0, packed * sizeof(float), h->stream);
        (void)hipMemsetAsync(l.b_packed, 0, bfl * sizeof(float), h->stream);
        a.w_packed = l.w_packed; a.b_packed = l.b_packed;
        if (kind == K_DENSE3 || kind == K_PW) {             // the split-f16 packs the network's GEMM-shaped layers run on
            const size_t halves = (size_t)(kind == K_DENSE3 ? 9 : 1) * ((cin + 7) / 8) * l.Npad * 8;
            if (l.ws_hi.reserve(halves) || l.ws_lo.reserve(halves)) { rc = 1; return; }
            (void)hipMemsetAsync(l.ws_hi, 0, l.ws_bytes(), h->stream);
            (void)hipMemsetAsync(l.ws_lo, 0, l.ws_bytes(), h->stream);
            a.ws_hi = l.ws_hi.get(); a.ws_lo = l.ws_lo.get(); a.w_ovf = h->range_flags + 2;
            (void)hipMemsetAsync(h->range_flags + 2, 0, sizeof(unsigned), h->stream);
        }
        launch_fold_pack(a, h->stream);
        if (l.ws_hi) {                                      // a weight outside the split's range: this operator runs on the f32-MFMA family
            unsigned wflag = 0;
            (void)hipMemcpyAsync(&wflag, h->range_flags + 2, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
            if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = 1; return; }
            if (wflag) { l.ws_hi.reset(); l.ws_lo.reset(); }
        }
    }
    ~TmpLayer() { (void)hipStreamSynchronize(h->stream); }      // then the packs go with l
};
}  // namespace

int yn_op_dwconv3x3(yn_handle* h, const float* x, int B, int H, int W, int C, int stride, const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if (C & 1) return fail(h, "yn_op_dwconv3x3: C must be even");
    TmpLayer t(h, K_DW, C, C, stride, act, w, bias);
    if (t.rc) return fail(h, "yn_op_dwconv3x3: out of memory");
    run_dw(h, t.l, x, C, 0, B, H, W, y, C, 0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_pwconv(yn_handle* h, const float* x, int B, int H, int W, int Cin, int Cout, const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if (Cin & 1) return fail(h, "yn_op_pwconv: Cin must be even");
    TmpLayer t(h, K_PW, Cin, Cout, 1, act, w, bias);
    if (t.rc) return fail(h, "yn_op_pwconv: out of memory");
    run_pw(h, t.l, x, Cin, 0, (long)B * H * W, y, Cout, 0, nullptr, 0, 0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_pwconv_group(yn_handle* h, int n, const float* const* x, const int* in_ld, const int* in_off, const int* M, const int* Cin, int Cout,
                       const float* const* w, const float* const* bias, int act, float* const* y, const int* out_ld, const int* out_off)
{
    YN_ENTER(h);
    if (n < 1 || n > YN_GROUP_MAX) return fail(h, "yn_op_pwconv_group: 1 to %d members", YN_GROUP_MAX);
    for (int p = 0; p < n; ++p)
        if ((Cin[p] & 1) || (in_ld[p] & 1) || (in_off[p] & 1) || M[p] < 1 || in_ld[p] < in_off[p] + Cin[p] || out_ld[p] < out_off[p] + Cout)
            return fail(h, "yn_op_pwconv_group: member %d: Cin, in_ld and in_off must be even, the rows inside their strides", p);
    std::unique_ptr<TmpLayer> t[YN_GROUP_MAX];
    const Layer* l[YN_GROUP_MAX];
    GemmArgs a[YN_GROUP_MAX];
    for (int p = 0; p < n; ++p) {
        t[p].reset(new TmpLayer(h, K_PW, Cin[p], Cout, 1, act, w[p], bias ? bias[p] : nullptr));
        if (t[p]->rc) return fail(h, "yn_op_pwconv_group: out of memory");
        l[p] = &t[p]->l;
        a[p] = pw_args(h, t[p]->l, x[p], in_ld[p], in_off[p], M[p], y[p], out_ld[p], out_off[p], nullptr, 0, 0);
    }
    if (!run_pw_group(h, l, a, n, "op_group")) return fail(h, "yn_op_pwconv_group: the members do not run as one grouped launch (split packs, equal padded widths)");
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_pwconv_shuffle(yn_handle* h, const float* x, const float* pass, int B, int H, int W, int Cin, int Cout,
                         const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if ((Cin & 1) || (Cout & 1)) return fail(h, "yn_op_pwconv_shuffle: Cin and Cout must be even");
    if (!pass) return fail(h, "yn_op_pwconv_shuffle: null pass-through tensor");
    TmpLayer t(h, K_PW, Cin, Cout, 1, act, w, bias);
    if (t.rc) return fail(h, "yn_op_pwconv_shuffle: out of memory");
    run_pw(h, t.l, x, Cin, 0, (long)B * H * W, y, 2 * Cout, 0, pass, Cout, 0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_conv3x3(yn_handle* h, const float* x, const float* x2, int resample, int B, int H, int W, int Cin, int Cout,
                  const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if (Cin % 32) return fail(h, "yn_op_conv3x3: Cin must be a multiple of 32");
    if (resample && !x2) return fail(h, "yn_op_conv3x3: resample without x2");
    TmpLayer t(h, K_DENSE3, Cin, Cout, 1, act, w, bias);
    if (t.rc) return fail(h, "yn_op_conv3x3: out of memory");
    run_c3(h, t.l, x, x2, resample, B, H, W, y);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_stem(yn_handle* h, const float* x, int B, int H, int W, int Cout, const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if (Cout != 24) return fail(h, "yn_op_stem: Cout must be 24");
    TmpLayer t(h, K_STEM, 3, Cout, 2, act, w, bias);
    if (t.rc) return fail(h, "yn_op_stem: out of memory");
    {
        Bracket br(h, "op.stem", 2.0 * B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * 27 * Cout, 0.0);
        launch_stem(x, B, H, W, t.l.w_packed, t.l.b_packed, Cout, act, y, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_stem_pool(yn_handle* h, const float* x, int B, int H, int W, int Cout, const float* w, const float* bias, int act, float* y)
{
    YN_ENTER(h);
    if (Cout != 24) return fail(h, "yn_op_stem_pool: Cout must be 24");
    TmpLayer t(h, K_STEM, 3, Cout, 2, act, w, bias);
    if (t.rc) return fail(h, "yn_op_stem_pool: out of memory");
    {
        Bracket br(h, "op.stem+maxpool", 2.0 * B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * 27 * Cout, 0.0);
        launch_stem_pool(x, B, H, W, t.l.w_packed, t.l.b_packed, Cout, act, y, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_maxpool3x3s2(yn_handle* h, const float* x, int B, int H, int W, int C, float* y)
{
    YN_ENTER(h);
    if (C % 4) return fail(h, "yn_op_maxpool3x3s2: C must be a multiple of 4");
    h->cur = h->stream;
    {
        Bracket br(h, "op.maxpool", 0.0, 0.0);
        launch_maxpool(x, B, H, W, C, y, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_shuffle_block(yn_handle* h, const char* block, const float* x, int B, int H, int W, float* y)
{
    YN_ENTER(h);
    if (!h->folded) return fail(h, "yn_op_shuffle_block before yn_fold_bn");
    h->cur = h->stream;
    const std::string P = block;
    if (!h->by_name.count(P + ".b2.pw1")) return fail(h, "unknown block '%s'", block);
    const bool s2 = h->by_name.count(P + ".b1.dw") != 0;
    const Layer& pw1 = L(h, P + ".b2.pw1");
    const int bf = pw1.cout, C = 2 * bf;
    const int Cin = s2 ? pw1.cin : C;
    const int Ho = s2 ? (H - 1) / 2 + 1 : H, Wo = s2 ? (W - 1) / 2 + 1 : W;
    const long Mi = (long)B * H * W, Mo = (long)B * Ho * Wo;
    DevBuf<float> t1, t2, tdw, tb1;
    HIPCHK(h, t1.reserve((size_t)Mi * bf));
    HIPCHK(h, t2.reserve((size_t)Mo * bf));
    if (s2) {
        HIPCHK(h, tdw.reserve((size_t)Mo * Cin));
        HIPCHK(h, tb1.reserve((size_t)Mo * bf));
        run_dw(h, L(h, P + ".b1.dw"), x, Cin, 0, B, H, W, tdw, Cin, 0);
        run_pw(h, L(h, P + ".b1.pw"), tdw, Cin, 0, Mo, tb1, bf, 0, nullptr, 0, 0);
        run_pw(h, pw1, x, Cin, 0, Mi, t1, bf, 0, nullptr, 0, 0);
        run_dw(h, L(h, P + ".b2.dw"), t1, bf, 0, B, H, W, t2, bf, 0);
        run_pw(h, L(h, P + ".b2.pw2"), t2, bf, 0, Mo, y, C, 0, tb1, bf, 0);
    } else {
        run_unit(h, P, x, B, H, W, y, t1, t2);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// A stride-2 block as down_unit_pipe_kernel on any even map (the network only reaches maps that are multiples of 4 on this kernel: the
// ragged tile rows are reachable here alone).  An error where the kernel does not cover the block: there is no other path behind this entry.
int yn_op_down_unit(yn_handle* h, const char* block, const float* x, int B, int H, int W, float* y)
{
    YN_ENTER(h);
    if (!h->folded) return fail(h, "yn_op_down_unit before yn_fold_bn");
    h->cur = h->stream;
    const std::string P = block;
    if (!h->by_name.count(P + ".b2.pw1") || !h->by_name.count(P + ".b1.dw")) return fail(h, "'%s' is not a stride-2 block", block);
    const Layer &lp1 = L(h, P + ".b2.pw1"), &ldw = L(h, P + ".b2.dw"), &lp2 = L(h, P + ".b2.pw2"), &l1d = L(h, P + ".b1.dw"), &l1p = L(h, P + ".b1.pw");
    const int bf = lp1.cout, Cin = lp1.cin;
    DownArgs d{};
    d.x = x; d.cin = Cin;
    d.W1h = lp1.ws_hi; d.W1l = lp1.ws_lo; d.b1 = lp1.b_packed; d.act1 = lp1.act; d.Npad1 = lp1.Npad;
    d.wdw = ldw.w_packed; d.bdw = ldw.b_packed; d.dw_act = ldw.act;
    d.W2h = lp2.ws_hi; d.W2l = lp2.ws_lo; d.b2 = lp2.b_packed; d.act2 = lp2.act; d.Npad2 = lp2.Npad;
    d.wdw1 = l1d.w_packed; d.bdw1 = l1d.b_packed; d.dw1_act = l1d.act;
    d.W3h = l1p.ws_hi; d.W3l = l1p.ws_lo; d.b3 = l1p.b_packed; d.act3 = l1p.act; d.Npad3 = l1p.Npad;
    d.out = y; d.B = B; d.H = H; d.W = W; d.bf = bf;
    d.ovf = h->range_flags ? h->range_flags + 1 : nullptr;
    if (exact(h) || lp2.cin != bf || lp2.cout != bf || ldw.stride != 2 || l1d.stride != 2 || l1d.cout != Cin || l1p.cin != Cin || l1p.cout != bf || !down_unit_covers(d))
        return fail(h, "yn_op_down_unit: down_unit_pipe_kernel does not cover '%s' at %d x %d x %d (cin %d, branch width %d)", block, B, H, W, Cin, bf);
    {
        Bracket br(h, P + ".unit", 0.0, 0.0);
        launch_down_unit(d, h->cur);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// The candidate decode alone (decode_kernel<false, KMAX>): dense raw NHWC heads, row stride A(5+C) as for yn_score_full -> every candidate's
// box [B,N,4], best score [B,N] and class [B,N] (-1 below conf_thresh).
int yn_op_decode_cand(yn_handle* h, const float* h8, const float* h16, const float* h32, int B, float conf_thresh,
                      float* boxes, float* scores, int32_t* cls)
{
    YN_ENTER(h);
    if (B <= 0 || !h8 || !h16 || !h32 || !boxes || !scores || !cls) return fail(h, "yn_op_decode_cand: bad arguments");
    const float* const heads[3] = {h8, h16, h32};
    h->cur = h->stream;
    {
        Bracket br(h, "op.decode_cand", 0.0, 0.0);
        launch_decode_cand(heads, h->grid, B, conf_thresh, boxes, scores, cls, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The stretch of yn_infer's forward from the output of the heads' layer .1 to the candidate arrays, on caller-provided activations
// [B, H/8 (16, 32), W/8 (16, 32), 96] NHWC: run_head_tail with the handle's weights, switches and conf_thresh, the decode of the raw heads where
// no fused front end ran, then the handle's candidate arrays copied out.
int yn_op_head_tail(yn_handle* h, const float* x8, const float* x16, const float* x32, int B, float* boxes, float* scores, int32_t* cls)
{
    YN_ENTER(h);
    if (check_ready(h, B)) return 1;
    if (!x8 || !x16 || !x32 || !boxes || !scores || !cls) return fail(h, "yn_op_head_tail: null pointer");
    if (int rp = range_pending(h, "yn_op_head_tail")) return rp;
    GridInfo g = h->grid;
    g.head_ld = (h->head_ch + 3) & ~3;
    if (ensure_post(h, B, g.N, g.C) || ensure_heads(h, B)) return 1;
    h->cur = h->stream;
    DevBuf<float> tA, tC;
    const size_t rows = (size_t)B * (g.hw[0] + g.hw[1] + g.hw[2]);
    HIPCHK(h, tA.reserve(rows * NECK));
    HIPCHK(h, tC.reserve(rows * NECK));
    const float* const src[3] = {x8, x16, x32};
    float* const hA[3] = {tA, tA + (size_t)B * g.hw[0] * NECK, tA + (size_t)B * (g.hw[0] + g.hw[1]) * NECK};
    float* const hC[3] = {tC, tC + (size_t)B * g.hw[0] * NECK, tC + (size_t)B * (g.hw[0] + g.hw[1]) * NECK};
    float* const heads[3] = {h->heads_int[0], h->heads_int[1], h->heads_int[2]};
    const bool fuse_all = head_fuse_all(h, B, true);
    int rc = 0;
    if (heads_groupable(h)) rc = run_head_tail(h, -1, B, src, hA, hC, heads, g.head_ld, fuse_all);
    else
        for (int hd = 0; hd < 3 && !rc; ++hd) rc = run_head_tail(h, hd, B, src, hA, hC, heads, g.head_ld, fuse_all);
    if (!rc && !fuse_all) decode_raw_heads(h, heads, g, B);
    if (!rc) {
        const size_t n = (size_t)B * g.N;
        HIPCHK(h, hipMemcpyAsync(boxes, h->cand_boxes, n * 4 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(scores, h->cand_scores, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(cls, h->cand_cls, n * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));             // the scratch tensors go with this call
    return rc;
}

int yn_op_nchw_to_nhwc(yn_handle* h, const float* x, int B, int C, int H, int W, float* y)
{
    YN_ENTER(h);
    launch_nchw_to_nhwc(x, B, C, H, W, y, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_op_nhwc_to_nchw(yn_handle* h, const float* x, int B, int C, int H, int W, float* y)
{
    YN_ENTER(h);
    launch_nhwc_to_nchw(x, B, C, H, W, y, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- profiling ---------------------------------------------------------------------------------
int yn_profile_enable(yn_handle* h, int enable)
{
    YN_ENTER(h);
    h->profiling = enable != 0;
    h->prof.clear();
    h->event_next = 0;
    return 0;
}

int yn_profile_count(yn_handle* h) { return h ? (int)h->prof.size() : -1; }

int yn_profile_get(yn_handle* h, int i, char* name, int name_cap, char* kernel, int kernel_cap, float* ms,
                   double* alg_flops, double* alg_bytes)
{
    YN_ENTER(h);
    if (i < 0 || i >= (int)h->prof.size()) return fail(h, "yn_profile_get: index %d out of range", i);
    const ProfRec& r = h->prof[i];
    HIPCHK(h, hipEventSynchronize(r.e1));
    float t = 0.0f;
    HIPCHK(h, hipEventElapsedTime(&t, r.e0, r.e1));
    if (name && name_cap > 0) { strncpy(name, r.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (kernel && kernel_cap > 0) { strncpy(kernel, r.kernel.c_str(), kernel_cap - 1); kernel[kernel_cap - 1] = 0; }
    if (ms) *ms = t;
    if (alg_flops) *alg_flops = r.flops;
    if (alg_bytes) *alg_bytes = r.bytes;
    return 0;
}

// ---- VOC mAP (kernels_eval.hip) ---------------------------------------------------------------------------------------------
int yn_eval_create(yn_handle* h, int num_classes, double ovthresh, yn_eval** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_eval_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::EvalState* st = nullptr;
    if (ynk::eval_create(h->cfg.device, num_classes, ovthresh, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_eval{st};
    return 0;
}

void yn_eval_destroy(yn_eval* e)
{
    if (!e) return;
    ynk::eval_destroy(e->st);
    delete e;
}

#define YN_EVAL_CALL(call)                                                   \
    do {                                                                     \
        std::string err;                                                     \
        const int rc_ = (call);                                              \
        if (rc_ == 1) return fail(h, "%s", err.c_str());                     \
        if (rc_ == YN_STATUS_RANGE) { h->err = err; return YN_STATUS_RANGE; } \
        return 0;                                                            \
    } while (0)

int yn_eval_reset(yn_handle* h, yn_eval* e)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_eval_reset: null evaluator");
    YN_EVAL_CALL(ynk::eval_reset(e->st, h->stream, err));
}

int yn_eval_add(yn_handle* h, yn_eval* e, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom_host,
                const int32_t* gt_host, const int32_t* gt_offsets_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_eval_add: null evaluator");
    YN_EVAL_CALL(ynk::eval_add(e->st, h->stream, B, rec_dev, offsets_dev, geom_host, gt_host, gt_offsets_host, err));
}

int yn_eval_finish(yn_handle* h, yn_eval* e, int use_07_metric, double* ap_host, int64_t* npos_host, int64_t* ndet_host)
{
    YN_ENTER(h);
    if (!e || !ap_host) return fail(h, "yn_eval_finish: null argument");
    YN_EVAL_CALL(ynk::eval_finish(e->st, h->stream, use_07_metric, ap_host, npos_host, ndet_host, err));
}

int yn_eval_curve(yn_handle* h, yn_eval* e, int cls, double* rec_host, double* prec_host, int64_t cap)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_eval_curve: null evaluator");
    YN_EVAL_CALL(ynk::eval_curve(e->st, h->stream, cls, rec_host, prec_host, cap, err));
}

int yn_eval_records(yn_handle* h, yn_eval* e, int32_t* host, int64_t cap)
{
    YN_ENTER(h);
    if (!e || !host) return fail(h, "yn_eval_records: null argument");
    YN_EVAL_CALL(ynk::eval_records(e->st, h->stream, host, cap, err));
}

int yn_eval_size(yn_eval* e, int64_t* records, int64_t* images)
{
    if (!e) return 1;
    ynk::eval_size(e->st, records, images);
    return 0;
}

// ---- COCO box AP (kernels_coco.hip) -----------------------------------------------------------------------------------------
int yn_coco_create(yn_handle* h, int num_classes, int max_det, yn_coco** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_coco_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::CocoState* st = nullptr;
    if (ynk::coco_create(h->cfg.device, num_classes, max_det, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_coco{st};
    return 0;
}

void yn_coco_destroy(yn_coco* e)
{
    if (!e) return;
    ynk::coco_destroy(e->st);
    delete e;
}

int yn_coco_reset(yn_handle* h, yn_coco* e)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_coco_reset: null evaluator");
    YN_EVAL_CALL(ynk::coco_reset(e->st, h->stream, err));
}

int yn_coco_add(yn_handle* h, yn_coco* e, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom_host,
                const int64_t* image_ids_host, const double* gt_host, const int32_t* gt_meta_host, const int32_t* gt_offsets_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_coco_add: null evaluator");
    YN_EVAL_CALL(ynk::coco_add(e->st, h->stream, B, rec_dev, offsets_dev, geom_host, image_ids_host, gt_host, gt_meta_host, gt_offsets_host, err));
}

int yn_coco_finish(yn_handle* h, yn_coco* e, const double* iou_thrs_host, int num_iou, const double* rec_thrs_host, int num_rec,
                   const double* area_rng_host, int num_area, const int32_t* max_dets_host, int num_max_dets, double* precision_host,
                   double* recall_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_coco_finish: null evaluator");
    YN_EVAL_CALL(ynk::coco_finish(e->st, h->stream, iou_thrs_host, num_iou, rec_thrs_host, num_rec, area_rng_host, num_area, max_dets_host,
                                  num_max_dets, precision_host, recall_host, err));
}

int yn_coco_matches(yn_handle* h, yn_coco* e, float* det_host, int64_t* seg_host, uint32_t* flags_host, int num_area)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_coco_matches: null evaluator");
    YN_EVAL_CALL(ynk::coco_matches(e->st, h->stream, det_host, seg_host, flags_host, num_area, err));
}

int yn_coco_size(yn_coco* e, int64_t* detections, int64_t* images)
{
    if (!e) return 1;
    ynk::coco_size(e->st, detections, images);
    return 0;
}

// ---- anchor-box k-means (kernels_kmeans.hip) -------------------------------------------------------------------------------------
int yn_kmeans_create(yn_handle* h, int64_t capacity, int max_k, yn_kmeans** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_kmeans_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::KmeansState* st = nullptr;
    if (ynk::kmeans_create(h->cfg.device, capacity, max_k, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_kmeans{st};
    return 0;
}

void yn_kmeans_destroy(yn_kmeans* e)
{
    if (!e) return;
    ynk::kmeans_destroy(e->st);
    delete e;
}

int yn_kmeans_set_boxes(yn_handle* h, yn_kmeans* e, const double* wh_dev, int64_t n)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_set_boxes: null object");
    YN_EVAL_CALL(ynk::kmeans_set_boxes(e->st, h->stream, wh_dev, n, err));
}

int yn_kmeans_seed(yn_handle* h, yn_kmeans* e, int k, int64_t first_index, const double* u_host, double* centroids_host, int32_t* picked_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_seed: null object");
    YN_EVAL_CALL(ynk::kmeans_seed(e->st, h->stream, k, first_index, u_host, centroids_host, picked_host, err));
}

int yn_kmeans_set_centroids(yn_handle* h, yn_kmeans* e, const double* wh_host, int k)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_set_centroids: null object");
    YN_EVAL_CALL(ynk::kmeans_set_centroids(e->st, h->stream, wh_host, k, err));
}

int yn_kmeans_run(yn_handle* h, yn_kmeans* e, double loss_convergence, int iters, double* centroids_host, int64_t* counts_host,
                  double* loss_host, int32_t* iterations_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_run: null object");
    YN_EVAL_CALL(ynk::kmeans_run(e->st, h->stream, loss_convergence, iters, centroids_host, counts_host, loss_host, iterations_host, err));
}

int yn_kmeans_pass(yn_handle* h, yn_kmeans* e, double* centroids_host, int64_t* counts_host, double* loss_host)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_pass: null object");
    YN_EVAL_CALL(ynk::kmeans_pass(e->st, h->stream, centroids_host, counts_host, loss_host, err));
}

int yn_kmeans_assign(yn_handle* h, yn_kmeans* e, int32_t* group_dev)
{
    YN_ENTER(h);
    if (!e) return fail(h, "yn_kmeans_assign: null object");
    YN_EVAL_CALL(ynk::kmeans_assign(e->st, h->stream, group_dev, err));
}

int yn_kmeans_stats(yn_kmeans* e, int64_t* passes, int64_t* host_reads)
{
    if (!e) return 1;
    ynk::kmeans_stats(e->st, passes, host_reads);
    return 0;
}

// ---- detections painted onto frames (kernels_draw.hip; test.py:50-92) ---------------------------------------------------------------
static_assert(YN_DRAW_LETTERBOX == 0 && YN_DRAW_PIXELS == 1, "yn_draw_batch spaces");

int yn_draw_create(yn_handle* h, int num_classes, const uint8_t* colors_host, const char* const* labels_host, const uint8_t* atlas_host, int gw, int gh,
                   int thickness, yn_draw** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_draw_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::DrawState* st = nullptr;
    if (ynk::draw_create(h->cfg.device, num_classes, colors_host, labels_host, atlas_host, gw, gh, thickness, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_draw{st};
    return 0;
}

void yn_draw_destroy(yn_draw* d)
{
    if (!d) return;
    ynk::draw_destroy(d->st);
    delete d;
}

int yn_draw_batch(yn_handle* h, yn_draw* d, int B, uint8_t* const* frames_host, const int32_t* geom_host, int space, const float* rec_dev,
                  const int32_t* offsets_dev, int64_t rec_capacity, float vis_thresh)
{
    YN_ENTER(h);
    if (!d) return fail(h, "yn_draw_batch: null object");
    if (ynk::draw_device(d->st) != h->cfg.device)
        return fail(h, "yn_draw_batch: the object was made for device %d, the handle is on device %d", ynk::draw_device(d->st), h->cfg.device);
    YN_EVAL_CALL(ynk::draw_batch(d->st, h->stream, B, frames_host, geom_host, space, rec_dev, offsets_dev, rec_capacity, vis_thresh, err));
}

int yn_draw_status(yn_handle* h, yn_draw* d, int64_t* drawn, int64_t* skipped, int* range_mark)
{
    YN_ENTER(h);
    if (!d) return fail(h, "yn_draw_status: null object");
    YN_EVAL_CALL(ynk::draw_status(d->st, h->stream, drawn, skipped, range_mark, err));
}

int yn_draw_prims(yn_handle* h, yn_draw* d, int32_t* host, int64_t cap)
{
    YN_ENTER(h);
    if (!d || (!host && cap > 0)) return fail(h, "yn_draw_prims: null argument");
    YN_EVAL_CALL(ynk::draw_prims(d->st, h->stream, host, cap, err));
}

// ---- detections cut out of frames as chips (kernels_chip.hip) --------------------------------------------------------------------
static_assert(sizeof(yn_chip_params) == 17 * 4 && offsetof(yn_chip_params, min_score) == 7 * 4, "yn_chip_params: seven int32, then ten floats");
static_assert(YN_CHIP_LETTERBOX == 0 && YN_CHIP_STRETCH == 1 && YN_CHIP_U8 == 0 && YN_CHIP_F32 == 1, "yn_chip_params fits and formats");

int yn_chip_create(yn_handle* h, int num_classes, const uint8_t* class_keep_host, int max_chips, const yn_chip_params* p, yn_chip** out)
{
    YN_ENTER(h);
    if (!out || !p) return fail(h, "yn_chip_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::ChipState* st = nullptr;
    if (ynk::chip_create(h->cfg.device, num_classes, class_keep_host, max_chips, &p->cw, &p->min_score, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_chip{st};
    return 0;
}

void yn_chip_destroy(yn_chip* c)
{
    if (!c) return;
    ynk::chip_destroy(c->st);
    delete c;
}

int yn_chip_batch(yn_handle* h, yn_chip* c, int B, const uint8_t* const* frames_host, const int32_t* geom_host, int space, const float* rec_dev,
                  const int32_t* offsets_dev, int64_t rec_capacity, void* chips_dev, int32_t* index_dev, int32_t* rect_dev, int32_t* chip_offsets_dev)
{
    YN_ENTER(h);
    if (!c) return fail(h, "yn_chip_batch: null object");
    YN_EVAL_CALL(ynk::chip_batch(c->st, h->cfg.device, h->stream, B, frames_host, geom_host, space, rec_dev, offsets_dev, rec_capacity, chips_dev, index_dev,
                                 rect_dev, chip_offsets_dev, err));
}

int yn_chip_status(yn_handle* h, yn_chip* c, int64_t counters_host[4])
{
    YN_ENTER(h);
    if (!c || !counters_host) return fail(h, "yn_chip_status: null argument");
    YN_EVAL_CALL(ynk::chip_status(c->st, h->stream, counters_host, err));
}

// ---- detections tracked across frames (kernels_track.hip) ---------------------------------------------------------------------
static_assert(sizeof(yn_track_params) == 11 * 4 && offsetof(yn_track_params, max_lost) == 8 * 4, "yn_track_params: eight floats, then three int32");

int yn_track_create(yn_handle* h, int streams, int max_tracks, int max_dets, const yn_track_params* p, yn_track** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_track_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::TrackState* st = nullptr;
    if (ynk::track_create(h->cfg.device, h->stream, streams, max_tracks, max_dets, p ? &p->track_high : nullptr, p ? &p->max_lost : nullptr, &st, err))
        return fail(h, "%s", err.c_str());
    *out = new yn_track{st};
    return 0;
}

void yn_track_destroy(yn_track* t)
{
    if (!t) return;
    ynk::track_destroy(t->st);
    delete t;
}

#define YN_TRACK_ENTER(name)                                                                                         \
    YN_ENTER(h);                                                                                                     \
    if (!t) return fail(h, name ": null object");                                                                    \
    if (ynk::track_device(t->st) != h->cfg.device)                                                                   \
        return fail(h, name ": the object was made for device %d, the handle is on device %d", ynk::track_device(t->st), h->cfg.device)

int yn_track_reset(yn_handle* h, yn_track* t, int stream)
{
    YN_TRACK_ENTER("yn_track_reset");
    YN_EVAL_CALL(ynk::track_reset(t->st, h->stream, stream, err));
}

int yn_track_update(yn_handle* h, yn_track* t, int B, const int32_t* stream_host, const float* rec_dev, const int32_t* offsets_dev, int64_t rec_capacity,
                    float* out_rec_dev, int32_t* out_ids_dev, int32_t* out_offsets_dev)
{
    YN_TRACK_ENTER("yn_track_update");
    YN_EVAL_CALL(ynk::track_update(t->st, h->stream, B, stream_host, rec_dev, offsets_dev, rec_capacity, out_rec_dev, out_ids_dev, out_offsets_dev, err));
}

int yn_track_state(yn_handle* h, yn_track* t, int stream, int32_t* meta_host, float* filt_host, int32_t* next_id)
{
    YN_TRACK_ENTER("yn_track_state");
    YN_EVAL_CALL(ynk::track_state(t->st, h->stream, stream, meta_host, filt_host, next_id, err));
}

int yn_track_status(yn_handle* h, yn_track* t, int64_t counters_host[6])
{
    YN_TRACK_ENTER("yn_track_status");
    if (!counters_host) return fail(h, "yn_track_status: null argument");
    YN_EVAL_CALL(ynk::track_status(t->st, h->stream, counters_host, err));
}

// ---- the merge lists of yn_tta and yn_slice (struct MergeLists above) ------------------------------------------------------------
void MergeLists::reserve(Reserve& take, const yn_config& cfg, int units_, int cap_)
{
    device = cfg.device; A = cfg.num_anchors; C = cfg.num_classes; units = units_; cap = cap_;
    state_host.resize(MERGE_STATE + units);
    const size_t lN = (size_t)units * cap;
    take(lb, lN * 4); take(ls, lN); take(lc, lN);
    take(state, (size_t)MERGE_STATE + units);
    take(mb, lN * 4); take(ms, lN); take(mc, lN); take(mcount, (size_t)units);
    take(rec, lN * 6); take(offsets, (size_t)units + 1);
}

// the lists' unused rows are never candidates (class -1, set by open()), but the NMS kernels may load them: finite values once
bool MergeLists::clear_once(hipStream_t s)
{
    const size_t lN = (size_t)units * cap;
    return hipMemsetAsync(lb, 0, lN * 4 * sizeof(float), s) == hipSuccess && hipMemsetAsync(ls, 0, lN * sizeof(float), s) == hipSuccess &&
           hipStreamSynchronize(s) == hipSuccess;
}

int MergeLists::belongs(yn_handle* h, const char* who) const
{
    if (device != h->cfg.device || A != h->cfg.num_anchors || C != h->cfg.num_classes)
        return fail(h, "%s: the object was made for device %d, %d anchors, %d classes; the handle has %d, %d, %d", who, device, A, C, h->cfg.device,
                    h->cfg.num_anchors, h->cfg.num_classes);
    return 0;
}

// n empty lists (lists_n is the caller's: the lists count as valid once they have been appended to)
int MergeLists::open(yn_handle* h, int n)
{
    HIPCHK(h, hipMemsetAsync(state, 0, (MERGE_STATE + n) * sizeof(int32_t), h->stream));
    if (n > 0) HIPCHK(h, hipMemsetAsync(lc, 0xFF, (size_t)n * cap * sizeof(int32_t), h->stream));      // class -1: not a candidate (bucket_kernel)
    return 0;
}

// n filled lists -> ONE read-back (sizes, overflow flag, range mark), per-class NMS in yn_nms_merge's arithmetic (never DIoU), yn_pack_detections into
// rec / offsets.  `unit` names a list's owner in the overflow message; lists_n is n once the lists have been read, before any refusal.
int MergeLists::set_rule(yn_handle* h, const char* who, int rule_, int expected_)
{
    if (rule_ != YN_MERGE_NMS && rule_ != YN_MERGE_WBF) return fail(h, "%s: rule %d is neither YN_MERGE_NMS (0) nor YN_MERGE_WBF (1)", who, rule_);
    if (expected_ < 0) return fail(h, "%s: expected is %d (0 = the object's default, else the expected votes, at least 1)", who, expected_);
    rule = rule_; expected = expected_;
    return 0;
}

int MergeLists::set_soft(yn_handle* h, const char* who, int method, float sigma, float score_floor)
{
    if (soft_params(h, who, YN_SOFT_OFF, method, sigma, score_floor)) return 1;
    soft = method; soft_sigma = sigma; soft_floor = score_floor;
    return 0;
}

int MergeLists::merge(yn_handle* h, const char* who, const char* unit, int n, float nms_thresh, int default_expected)
{
    int32_t* st = state_host.data();
    HIPCHK(h, hipMemcpyAsync(st, state, (MERGE_STATE + n) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    lists_n = n;
    if (st[2] || range_pending(h, who)) {
        fail(h, "%s: a forward split an activation >= 65504 (split-f16 range): nothing is delivered - call yn_range_status to acknowledge, "
                "then yn_exact_f32(h, 1) and run again", who);
        return YN_STATUS_RANGE;
    }
    if (st[0]) {
        int worst = 0;
        for (int b = 0; b < n; ++b) if (st[MERGE_STATE + b] > cap) { worst = b; break; }
        return fail(h, "%s: the merge list of %s %d needs %d rows, list_capacity is %d (the largest list of the batch needs %d)", who, unit, worst,
                    st[MERGE_STATE + worst], cap, st[1]);
    }
    if (st[3]) {
        const int worst = 4095 - (st[3] >> 19);
        return fail(h, "%s: %s %d was appended %d rows whose class is not an integer in 0..%d", who, unit, worst, st[3] & ((1 << 19) - 1), C - 1);
    }
    const bool soft_on = rule == YN_MERGE_NMS && soft != YN_SOFT_OFF;      // (the setting is kept but unused under the WBF rule)
    if (rule == YN_MERGE_WBF ? ensure_wbf(h, n, cap, C) : (soft_on ? ensure_soft(h, n, cap, C) : ensure_post(h, n, cap, C))) return 1;
    NmsWork wk = h->nms;
    wk.ovf = nullptr; wk.ovf_host = nullptr;
    if (rule == YN_MERGE_WBF) {
        const int e = expected > 0 ? expected : (default_expected > 0 ? default_expected : 1);
        launch_wbf_pipeline(lb, ls, lc, n, cap, C, nms_thresh, e, wk, h->wbf, mb, ms, mc, nullptr, nullptr, nullptr, mcount, h->stream);
    } else if (soft_on) {
        launch_soft_pipeline(lb, ls, lc, n, cap, C, soft, nms_thresh, soft_sigma, soft_floor, wk, h->soft, mb, ms, mc, nullptr, mcount, h->stream);
    } else {
        launch_nms_pipeline(lb, ls, lc, n, cap, C, nms_thresh, 0, wk, mb, ms, mc, nullptr, mcount, h->stream);
    }
    launch_pack(mb, ms, mc, mcount, n, cap, rec, offsets, h->stream);
    HIPCHK(h, hipGetLastError());
    last_n = n;
    return 0;
}

// nothing to merge: n empty results (offsets[0 .. n] = 0)
int MergeLists::empty_result(yn_handle* h, int n)
{
    HIPCHK(h, hipMemsetAsync(offsets, 0, (size_t)(n + 1) * sizeof(int32_t), h->stream));
    last_n = n; lists_n = n; total = 0;
    return 0;
}

int MergeLists::result(const float** rec_dev, const int32_t** offsets_dev, int32_t* total_out)
{
    if (last_n < 0) return 1;
    if (rec_dev) *rec_dev = rec;
    if (offsets_dev) *offsets_dev = offsets;
    if (total_out) {
        if (total < 0) {
            DeviceScope on(device);
            int32_t v = 0;
            if (hipMemcpyAsync(&v, offsets + last_n, sizeof(int32_t), hipMemcpyDeviceToHost, last_stream) != hipSuccess ||
                hipStreamSynchronize(last_stream) != hipSuccess)
                return 1;
            total = v;
        }
        *total_out = total;
    }
    return 0;
}

// the first n lists and their sizes to host arrays (null: skipped), enqueued on the handle's stream: the caller synchronises
int MergeLists::copy_lists(yn_handle* h, int n, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host) const
{
    const size_t lN = (size_t)n * cap;
    if (boxes_host) HIPCHK(h, hipMemcpyAsync(boxes_host, lb, lN * 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (scores_host) HIPCHK(h, hipMemcpyAsync(scores_host, ls, lN * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (cls_host) HIPCHK(h, hipMemcpyAsync(cls_host, lc, lN * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (count_host) HIPCHK(h, hipMemcpyAsync(count_host, state + MERGE_STATE, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// ---- test-time augmentation for whole batches (kernels_tta.hip; utils/misc.py:90-148) ----------------------------------------------
int yn_resize_batch(yn_handle* h, const float* x_dev, int B, int S0, int s, int flip_pairs, float* out_dev)
{
    YN_ENTER(h);
    if (B < 0 || S0 < 1 || s < 1 || S0 > 16384 || s > 16384) return fail(h, "yn_resize_batch: bad extent (B %d, %d -> %d; sides 1..16384)", B, S0, s);
    if (B == 0) return 0;
    if (!x_dev || !out_dev) return fail(h, "yn_resize_batch: null argument");
    if (B > 21845) return fail(h, "yn_resize_batch: %d images exceed the launch grid (21845: one plane per grid row)", B);
    launch_tta_resize(x_dev, B, S0, s, flip_pairs != 0, out_dev, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

void yn_tta_destroy(yn_tta* t)
{
    if (!t) return;
    DeviceScope on(t->m.device);
    if (t->m.last_stream || t->m.lists_n >= 0) (void)hipDeviceSynchronize();      // (an object no call has launched on has nothing in flight)
    delete t;
}

int yn_tta_create(yn_handle* h, const int32_t* scales, int num_scales, int flip, int max_batch, int list_capacity, yn_tta** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_tta_create: null argument");
    *out = nullptr;
    if (!scales || num_scales < 1 || num_scales > 64) return fail(h, "yn_tta_create: 1..64 scales (got %d)", num_scales);
    for (int i = 0; i < num_scales; ++i) {
        if (scales[i] <= 0 || scales[i] % 32 || scales[i] > 4096) return fail(h, "yn_tta_create: scale %d is not a positive multiple of 32 up to 4096", scales[i]);
        if (i && scales[i] <= scales[i - 1]) return fail(h, "yn_tta_create: scales must ascend (%d after %d)", scales[i], scales[i - 1]);
    }
    if (max_batch < 1 || max_batch > 4096) return fail(h, "yn_tta_create: max_batch %d outside 1..4096", max_batch);
    if (list_capacity < 1 || list_capacity > nms_max_segment())
        return fail(h, "yn_tta_create: list_capacity %d outside 1..%d (the largest list the merge's NMS takes)", list_capacity, nms_max_segment());
    yn_tta* t = new yn_tta();
    t->flip = flip != 0; t->max_batch = max_batch;
    t->scales.assign(scales, scales + num_scales);
    t->smax = scales[num_scales - 1];
    t->Nmax = h->cfg.num_anchors * ((t->smax / 8) * (t->smax / 8) + (t->smax / 16) * (t->smax / 16) + (t->smax / 32) * (t->smax / 32));
    const size_t nb = (size_t)(t->flip ? 2 : 1) * max_batch, forwards = (size_t)(t->flip ? 2 : 1) * num_scales;
    Reserve take;
    take(t->xr, nb * 3 * t->smax * t->smax);
    t->f.reserve(take, nb, (size_t)t->Nmax);
    take(t->fstart, forwards * max_batch);
    t->m.reserve(take, h->cfg, max_batch, list_capacity);
    if (take.rc) {
        (void)hipGetLastError();
        const int smax = t->smax;
        yn_tta_destroy(t);
        return fail(h, "yn_tta_create: out of device memory (%zu bytes for %d images, %d scales up to %d, %d rows per list)", take.failed, max_batch,
                    num_scales, smax, list_capacity);
    }
    if (!t->m.clear_once(h->stream)) {
        yn_tta_destroy(t);
        return fail(h, "yn_tta_create: clearing the merge lists failed");
    }
    *out = t;
    return 0;
}

int yn_tta_infer(yn_handle* h, yn_tta* t, const float* x_dev, int B, int S0, float nms_thresh)
{
    YN_ENTER(h);
    if (!t) return fail(h, "yn_tta_infer: null object");
    if (need_square_grid(h, "yn_tta_infer")) return 1;      // (before anything of the object's is touched: the grid stays as it was found)
    MergeLists& m = t->m;
    m.drop_result(); m.lists_n = -1;
    if (m.belongs(h, "yn_tta_infer")) return 1;
    if (B < 0 || B > t->max_batch) return fail(h, "yn_tta_infer: %d images, the object's max_batch is %d", B, t->max_batch);
    const int nb = t->flip ? 2 * B : B;
    if (nb > h->cfg.max_batch)
        return fail(h, "yn_tta_infer: %d images%s need a handle with max_batch >= %d, this one has max_batch %d", B, t->flip ? " with their mirrors" : "", nb,
                    h->cfg.max_batch);
    m.last_stream = h->stream;
    if (B == 0) return m.empty_result(h, 0);
    if (!x_dev || S0 < 1 || S0 > 16384) return fail(h, "yn_tta_infer: bad input (side %d)", S0);
    if (check_ready(h, B)) return 1;
    if (int rp = range_pending(h, "yn_tta_infer")) return rp;
    const int S_prev = h->grid.S;
    struct Restore { yn_handle* h; int S; ~Restore() { if (h->grid.S != S) (void)yn_set_grid(h, S); } } restore{h, S_prev};      // the grid that was set before the call
    if (m.open(h, B)) return 1;
    for (size_t si = 0; si < t->scales.size(); ++si) {
        const int s = t->scales[si];
        launch_tta_resize(x_dev, B, S0, s, t->flip, t->xr, h->stream);
        HIPCHK(h, hipGetLastError());
        if (yn_set_grid(h, s)) return 1;
        const int N = h->grid.N;
        if (N > t->Nmax) return fail(h, "yn_tta_infer: %d predictions at %d exceed the object's %d", N, s, t->Nmax);
        if (int rc = yn_infer(h, t->xr, nb, t->f.fb, t->f.fs, t->f.fc, nullptr, t->f.fcount)) return rc;
        launch_tta_append(t->f.fb, t->f.fs, t->f.fc, t->f.fcount, B, N, t->flip, m.cap, t->max_batch, (int)si * (t->flip ? 2 : 1), m.lb, m.ls, m.lc, m.state,
                          t->fstart, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    return m.merge(h, "yn_tta_infer", "image", B, nms_thresh, (int)t->scales.size() * (t->flip ? 2 : 1));
}

int yn_merge_rule_tta(yn_handle* h, yn_tta* t, int rule, int expected)
{
    YN_ENTER(h);
    if (!t) return fail(h, "yn_merge_rule_tta: null object");
    return t->m.set_rule(h, "yn_merge_rule_tta", rule, expected);
}

int yn_merge_soft_tta(yn_handle* h, yn_tta* t, int method, float sigma, float score_floor)
{
    YN_ENTER(h);
    if (!t) return fail(h, "yn_merge_soft_tta: null object");
    return t->m.set_soft(h, "yn_merge_soft_tta", method, sigma, score_floor);
}

int yn_tta_result(yn_tta* t, const float** rec_dev, const int32_t** offsets_dev, int32_t* total)
{
    return t ? t->m.result(rec_dev, offsets_dev, total) : 1;
}

int yn_tta_forwards(yn_handle* h, yn_tta* t, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host, int32_t* forward_start_host)
{
    YN_ENTER(h);
    if (!t) return fail(h, "yn_tta_forwards: null object");
    if (t->m.lists_n < 0) return fail(h, "yn_tta_forwards: no yn_tta_infer has filled the lists");
    const int B = t->m.lists_n;
    if (B == 0) return 0;
    const size_t forwards = t->scales.size() * (t->flip ? 2 : 1);
    if (t->m.copy_lists(h, B, boxes_host, scores_host, cls_host, count_host)) return 1;
    if (forward_start_host)
        for (size_t f = 0; f < forwards; ++f)
            HIPCHK(h, hipMemcpyAsync(forward_start_host + f * B, t->fstart + f * t->max_batch, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- sliced inference: tiles of large frames on the device, merged per frame (kernels_slice.hip) ------------------------------
namespace {

// the checks every entry makes on rows t0 .. t0 + n - 1 of a tile table before anything is launched; F < 0: the caller holds no frame count
int slice_check(yn_handle* h, const char* who, int F, const uint8_t* const* frames, const int32_t* shapes, const int32_t* tiles, int t0, int n, int side)
{
    for (int t = t0; t < t0 + n; ++t) {
        const int32_t* r = tiles + (size_t)t * SLICE_ROW;
        if (r[0] < 0 || (F >= 0 && r[0] >= F)) return fail(h, "%s: tile %d names frame %d of %d", who, t, r[0], F < 0 ? 0 : F);
        const int h0 = shapes[2 * r[0]], w0 = shapes[2 * r[0] + 1];
        if (h0 < 1 || w0 < 1 || h0 > 16384 || w0 > 16384) return fail(h, "%s: tile %d: frame %d is %d x %d (sides 1..16384)", who, t, r[0], h0, w0);
        if (frames && !frames[r[0]]) return fail(h, "%s: tile %d: frame %d is a null pointer", who, t, r[0]);
        if (r[3] <= 0 || r[4] <= 0) return fail(h, "%s: tile %d has the non-positive extent %d x %d", who, t, r[4], r[3]);
        if (r[1] < 0 || r[2] < 0 || r[1] > w0 - r[3] || r[2] > h0 - r[4])
            return fail(h, "%s: tile %d, %d x %d at (%d, %d), lies outside its %d x %d frame", who, t, r[4], r[3], r[1], r[2], h0, w0);
        if (r[5] <= 0 || r[6] <= 0 || r[7] < 0 || r[8] < 0 || r[7] > side - r[5] || r[8] > side - r[6])
            return fail(h, "%s: tile %d has a bad letterbox geometry (%d x %d at (%d, %d) in %d)", who, t, r[6], r[5], r[7], r[8], side);
    }
    return 0;
}

int slice_object(yn_handle* h, const yn_slice* s, const char* who, int F)
{
    if (!s) return fail(h, "%s: null object", who);
    if (s->m.belongs(h, who)) return 1;
    if (F < 0 || F > s->m.units) return fail(h, "%s: %d frames, the object's max_frames is %d", who, F, s->m.units);
    return 0;
}

// a new table of T tiles over F frames: empty lists
int slice_clear(yn_handle* h, yn_slice* s, int F, int T)
{
    MergeLists& m = s->m;
    m.drop_result(); m.lists_n = -1; m.last_stream = h->stream;
    HIPCHK(h, s->tstart.reserve((size_t)(T > 0 ? T : 1), 256));
    HIPCHK(h, hipMemsetAsync(s->tstart, 0, (size_t)(T > 0 ? T : 1) * sizeof(int32_t), h->stream));
    if (m.open(h, F)) return 1;
    m.lists_n = F; s->lists_T = T; s->next_t = 0;
    return 0;
}

}  // namespace

void yn_slice_destroy(yn_slice* s)
{
    if (!s) return;
    DeviceScope on(s->m.device);
    (void)hipDeviceSynchronize();      // always: a yn_slice_infer that failed in its first forward has launched on x / f without leaving a mark in m
    delete s;
}

int yn_slice_create(yn_handle* h, int max_frames, int list_capacity, yn_slice** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_slice_create: null argument");
    *out = nullptr;
    if (max_frames < 1 || max_frames > 4096) return fail(h, "yn_slice_create: max_frames %d outside 1..4096", max_frames);
    if (list_capacity < 1 || list_capacity > nms_max_segment())
        return fail(h, "yn_slice_create: list_capacity %d outside 1..%d (the largest list the merge's NMS takes)", list_capacity, nms_max_segment());
    yn_slice* s = new yn_slice();
    Reserve take;
    s->m.reserve(take, h->cfg, max_frames, list_capacity);
    if (take.rc) {
        (void)hipGetLastError();
        yn_slice_destroy(s);
        return fail(h, "yn_slice_create: out of device memory (%zu bytes for %d frames, %d rows per list)", take.failed, max_frames, list_capacity);
    }
    if (!s->m.clear_once(h->stream)) {
        yn_slice_destroy(s);
        return fail(h, "yn_slice_create: clearing the merge lists failed");
    }
    *out = s;
    return 0;
}

int yn_slice_preprocess(yn_handle* h, int T, const uint8_t* const* frames, const int32_t* shapes, const int32_t* tiles, int side, const float* mean,
                        const float* stdv, float* x)
{
    YN_ENTER(h);
    if (T == 0) return 0;                                   // no tiles is not an error
    if (T < 0 || !frames || !shapes || !tiles || !x || !mean || !stdv) return fail(h, "yn_slice_preprocess: null pointer or negative tile count");
    if (side <= 0 || side > 16384) return fail(h, "yn_slice_preprocess: side %d outside 1..16384", side);
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_slice_preprocess: std must be positive");
    if (slice_check(h, "yn_slice_preprocess", -1, frames, shapes, tiles, 0, T, side)) return 1;
    launch_slice_tiles(T, frames, shapes, tiles, side, mean, stdv, x, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int yn_slice_append(yn_handle* h, yn_slice* s, int F, const int32_t* shapes, int T, const int32_t* tiles, int t0, int n, const float* out_boxes,
                    const float* out_scores, const int32_t* out_cls, const int32_t* count, int N, float edge_margin)
{
    YN_ENTER(h);
    if (slice_object(h, s, "yn_slice_append", F)) return 1;
    if (need_square_grid(h, "yn_slice_append")) return 1;
    if (T < 0 || t0 < 0 || n < 0 || t0 > T - n) return fail(h, "yn_slice_append: tiles %d .. %d of a table of %d", t0, t0 + n - 1, T);
    if (n > 0 && (!shapes || !tiles || !out_boxes || !out_scores || !out_cls || !count)) return fail(h, "yn_slice_append: null pointer");
    if (n > 0 && N < 1) return fail(h, "yn_slice_append: capacity %d per tile", N);
    if (n > 0 && ((uintptr_t)out_boxes & 15)) return fail(h, "yn_slice_append: out_boxes_dev must be 16-byte aligned (a box is loaded as one float4)");
    if (edge_margin != edge_margin) return fail(h, "yn_slice_append: edge_margin is not a number");
    MergeLists& m = s->m;
    if (t0 != 0 && (m.lists_n != F || s->lists_T != T || s->next_t != t0))
        return fail(h, "yn_slice_append: chunks go in table order - tile %d of %d over %d frames was expected next, got tile %d of %d over %d", s->next_t,
                    s->lists_T, m.lists_n, t0, T, F);
    if (slice_check(h, "yn_slice_append", F, nullptr, shapes, tiles, t0, n, h->grid.S)) return 1;
    if (t0 == 0 && slice_clear(h, s, F, T)) return 1;       // the first chunk opens the table
    m.drop_result(); m.last_stream = h->stream;
    if (n > 0 && F > 0) {
        launch_slice_append(F, shapes, tiles, t0, n, h->grid.S, out_boxes, out_scores, out_cls, count, N, m.cap, edge_margin, m.lb, m.ls, m.lc, m.state,
                            s->tstart, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    s->next_t = t0 + n;
    return 0;
}

int yn_slice_merge(yn_handle* h, yn_slice* s, int F, float nms_thresh)
{
    YN_ENTER(h);
    if (slice_object(h, s, "yn_slice_merge", F)) return 1;
    MergeLists& m = s->m;
    m.drop_result();
    if (m.lists_n != F) return fail(h, "yn_slice_merge: the lists hold %d frames, not %d (yn_slice_append from tile 0 first)", m.lists_n, F);
    m.last_stream = h->stream;
    if (F == 0) return m.empty_result(h, 0);
    return m.merge(h, "yn_slice_merge", "frame", F, nms_thresh, 1);
}

int yn_merge_rule_slice(yn_handle* h, yn_slice* s, int rule, int expected)
{
    YN_ENTER(h);
    if (!s) return fail(h, "yn_merge_rule_slice: null object");
    return s->m.set_rule(h, "yn_merge_rule_slice", rule, expected);
}

int yn_merge_soft_slice(yn_handle* h, yn_slice* s, int method, float sigma, float score_floor)
{
    YN_ENTER(h);
    if (!s) return fail(h, "yn_merge_soft_slice: null object");
    return s->m.set_soft(h, "yn_merge_soft_slice", method, sigma, score_floor);
}

int yn_slice_infer(yn_handle* h, yn_slice* s, int F, const uint8_t* const* frames, const int32_t* shapes, int T, const int32_t* tiles, const float* mean,
                   const float* stdv, float nms_thresh, float edge_margin)
{
    YN_ENTER(h);
    if (slice_object(h, s, "yn_slice_infer", F)) return 1;
    if (need_square_grid(h, "yn_slice_infer")) return 1;    // (before anything of the object's is touched)
    s->m.drop_result();
    if (T < 0) return fail(h, "yn_slice_infer: %d tiles", T);
    if (F == 0 || T == 0) {                                 // nothing to run: empty lists, F empty results
        if (slice_clear(h, s, F, 0)) return 1;
        return s->m.empty_result(h, F);
    }
    if (!frames || !shapes || !tiles || !mean || !stdv) return fail(h, "yn_slice_infer: null pointer");
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] > 0.0f)) return fail(h, "yn_slice_infer: std must be positive");
    if (edge_margin != edge_margin) return fail(h, "yn_slice_infer: edge_margin is not a number");
    if (check_ready(h, 1)) return 1;
    if (int rp = range_pending(h, "yn_slice_infer")) return rp;
    const int side = h->grid.S, N = h->grid.N, mb = h->cfg.max_batch;
    for (int f = 0; f < F; ++f)
        if (!frames[f]) return fail(h, "yn_slice_infer: frame %d is a null pointer", f);
    if (slice_check(h, "yn_slice_infer", F, frames, shapes, tiles, 0, T, side)) return 1;
    InferOut& o = s->f;
    if (s->x.cap() < (size_t)mb * 3 * side * side || o.fb.cap() < (size_t)mb * N * 4) HIPCHK(h, hipStreamSynchronize(h->stream));      // a block in use goes
    Reserve take;
    take(s->x, (size_t)mb * 3 * side * side);
    o.reserve(take, (size_t)mb, (size_t)N);
    if (take.rc) {
        (void)hipGetLastError();
        return fail(h, "yn_slice_infer: out of device memory (%zu bytes for %d tiles per forward at %d x %d): %s", take.failed, mb, side, side,
                    hipGetErrorString((hipError_t)take.rc));
    }
    for (int t0 = 0; t0 < T; t0 += mb) {
        const int n = T - t0 < mb ? T - t0 : mb;
        launch_slice_tiles(n, frames, shapes, tiles + (size_t)t0 * SLICE_ROW, side, mean, stdv, s->x, h->stream);
        HIPCHK(h, hipGetLastError());
        if (int rc = yn_infer(h, s->x, n, o.fb, o.fs, o.fc, nullptr, o.fcount)) return rc;
        if (int rc = yn_slice_append(h, s, F, shapes, T, tiles, t0, n, o.fb, o.fs, o.fc, o.fcount, N, edge_margin)) return rc;
    }
    return yn_slice_merge(h, s, F, nms_thresh);
}

int yn_slice_result(yn_slice* s, const float** rec_dev, const int32_t** offsets_dev, int32_t* total)
{
    return s ? s->m.result(rec_dev, offsets_dev, total) : 1;
}

int yn_slice_lists(yn_handle* h, yn_slice* s, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host, int32_t* tile_start_host)
{
    YN_ENTER(h);
    if (!s) return fail(h, "yn_slice_lists: null object");
    if (s->m.lists_n < 0) return fail(h, "yn_slice_lists: no yn_slice_append has filled the lists");
    const int F = s->m.lists_n;
    if (F > 0 && s->m.copy_lists(h, F, boxes_host, scores_host, cls_host, count_host)) return 1;
    if (tile_start_host && s->lists_T > 0)
        HIPCHK(h, hipMemcpyAsync(tile_start_host, s->tstart, (size_t)s->lists_T * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- record lists fused per unit: ensembles, or a TTA result with a sliced one (kernels_wbf.hip) ----------------------------------
void yn_fuse_destroy(yn_fuse* f)
{
    if (!f) return;
    DeviceScope on(f->m.device);
    (void)hipDeviceSynchronize();
    delete f;
}

int yn_fuse_create(yn_handle* h, int max_units, int list_capacity, yn_fuse** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_fuse_create: null argument");
    *out = nullptr;
    if (max_units < 1 || max_units > 4096) return fail(h, "yn_fuse_create: max_units %d outside 1..4096", max_units);
    if (list_capacity < 1 || list_capacity > nms_max_segment())
        return fail(h, "yn_fuse_create: list_capacity %d outside 1..%d (the largest list the merge takes)", list_capacity, nms_max_segment());
    yn_fuse* f = new yn_fuse();
    Reserve take;
    f->m.reserve(take, h->cfg, max_units, list_capacity);
    if (take.rc) {
        (void)hipGetLastError();
        yn_fuse_destroy(f);
        return fail(h, "yn_fuse_create: out of device memory (%zu bytes for %d units, %d rows per list)", take.failed, max_units, list_capacity);
    }
    if (!f->m.clear_once(h->stream)) {
        yn_fuse_destroy(f);
        return fail(h, "yn_fuse_create: clearing the merge lists failed");
    }
    *out = f;
    return 0;
}

static int fuse_object(yn_handle* h, const yn_fuse* f, const char* who, int B)
{
    if (!f) return fail(h, "%s: null object", who);
    if (f->m.belongs(h, who)) return 1;
    if (B < 0 || B > f->m.units) return fail(h, "%s: %d units, the object's max_units is %d", who, B, f->m.units);
    return 0;
}

int yn_fuse_open(yn_handle* h, yn_fuse* f, int B)
{
    YN_ENTER(h);
    if (fuse_object(h, f, "yn_fuse_open", B)) return 1;
    MergeLists& m = f->m;
    m.drop_result(); m.lists_n = -1; m.last_stream = h->stream;
    if (m.open(h, B)) return 1;
    m.lists_n = B; f->appends = 0;
    return 0;
}

int yn_fuse_append(yn_handle* h, yn_fuse* f, int B, const float* rec_dev, const int32_t* offsets_dev, float weight)
{
    YN_ENTER(h);
    if (fuse_object(h, f, "yn_fuse_append", B)) return 1;
    MergeLists& m = f->m;
    if (m.lists_n != B) return fail(h, "yn_fuse_append: the lists hold %d units, not %d (yn_fuse_open first)", m.lists_n, B);
    if (B > 0 && (!rec_dev || !offsets_dev)) return fail(h, "yn_fuse_append: null pointer");
    if (B > 0 && ((uintptr_t)rec_dev & 7)) return fail(h, "yn_fuse_append: rec_dev must be 8-byte aligned (a record is loaded as three float2)");
    if (weight != weight) return fail(h, "yn_fuse_append: weight is not a number");
    m.drop_result(); m.last_stream = h->stream;
    if (B > 0) {
        launch_fuse_append(rec_dev, offsets_dev, B, m.C, m.cap, weight, m.lb, m.ls, m.lc, m.state, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    ++f->appends;
    return 0;
}

int yn_fuse_merge(yn_handle* h, yn_fuse* f, int B, int rule, float thresh, int expected)
{
    YN_ENTER(h);
    if (fuse_object(h, f, "yn_fuse_merge", B)) return 1;
    MergeLists& m = f->m;
    m.drop_result();
    if (m.lists_n != B) return fail(h, "yn_fuse_merge: the lists hold %d units, not %d (yn_fuse_open first)", m.lists_n, B);
    if (m.set_rule(h, "yn_fuse_merge", rule, expected)) return 1;
    m.last_stream = h->stream;
    if (B == 0) return m.empty_result(h, 0);
    return m.merge(h, "yn_fuse_merge", "unit", B, thresh, f->appends);
}

int yn_merge_soft_fuse(yn_handle* h, yn_fuse* f, int method, float sigma, float score_floor)
{
    YN_ENTER(h);
    if (!f) return fail(h, "yn_merge_soft_fuse: null object");
    return f->m.set_soft(h, "yn_merge_soft_fuse", method, sigma, score_floor);
}

int yn_fuse_result(yn_fuse* f, const float** rec_dev, const int32_t** offsets_dev, int32_t* total)
{
    return f ? f->m.result(rec_dev, offsets_dev, total) : 1;
}

int yn_fuse_lists(yn_handle* h, yn_fuse* f, float* boxes_host, float* scores_host, int32_t* cls_host, int32_t* count_host)
{
    YN_ENTER(h);
    if (!f) return fail(h, "yn_fuse_lists: null object");
    if (f->m.lists_n < 0) return fail(h, "yn_fuse_lists: no yn_fuse_open has prepared the lists");
    const int B = f->m.lists_n;
    if (B > 0 && f->m.copy_lists(h, B, boxes_host, scores_host, cls_host, count_host)) return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- baseline JPEG decode: entropy stage on the host, the rest on the device (yn_jpeg_host.h, kernels_jpeg.hip) --------------------------
static_assert(YN_JPEG_OK == 0 && YN_JPEG_UNSUPPORTED == 1 && YN_JPEG_CORRUPT == 2 && YN_JPEG_TOO_LARGE == 3, "yn_jpeg statuses (yn_jpeg_host.h)");
static thread_local std::string g_jpeg_reason;      // of the calling thread's last yn_jpeg_info / yn_jpeg_coefficients

int yn_jpeg_info(const uint8_t* data, int64_t len, int32_t* info8)
{
    int32_t scratch[8];
    g_jpeg_reason.clear();
    return ynk::jpeg_info(data, len, info8 ? info8 : scratch, g_jpeg_reason);
}

int yn_jpeg_coefficients(const uint8_t* data, int64_t len, int16_t* coef_host, int64_t cap, uint16_t* qt_host, int32_t* grid_host, int32_t* status)
{
    int64_t needed = 0;
    g_jpeg_reason.clear();
    const int st = ynk::jpeg_coefficients(data, len, coef_host, cap, qt_host, grid_host, &needed, g_jpeg_reason);
    if (status) *status = st;
    return st;
}

int yn_jpeg_create(yn_handle* h, int max_batch, int64_t staging_bytes, int threads, yn_jpeg** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_jpeg_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::JpegState* st = nullptr;
    if (ynk::jpeg_create(h->cfg.device, max_batch, staging_bytes, threads, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_jpeg{st};
    return 0;
}

void yn_jpeg_destroy(yn_jpeg* j)
{
    if (!j) return;
    ynk::jpeg_destroy(j->st);
    delete j;
}

int yn_jpeg_decode_batch(yn_handle* h, yn_jpeg* j, int n, const uint8_t* const* data_host, const int64_t* len_host, uint8_t* const* frames_host,
                         int32_t* status_host, int32_t* failed)
{
    YN_ENTER(h);
    if (!j) return fail(h, "yn_jpeg_decode_batch: null object");
    if (ynk::jpeg_device(j->st) != h->cfg.device)
        return fail(h, "yn_jpeg_decode_batch: the object was made for device %d, the handle is on device %d", ynk::jpeg_device(j->st), h->cfg.device);
    YN_EVAL_CALL(ynk::jpeg_decode_batch(j->st, h->stream, n, data_host, len_host, frames_host, status_host, failed, err));
}

const char* yn_jpeg_reason(yn_jpeg* j, int i) { return j ? ynk::jpeg_reason(j->st, i) : g_jpeg_reason.c_str(); }

int yn_jpeg_timing(yn_handle* h, yn_jpeg* j, float* ms3)
{
    YN_ENTER(h);
    if (!j || !ms3) return fail(h, "yn_jpeg_timing: null argument");
    YN_EVAL_CALL(ynk::jpeg_timing(j->st, ms3, err));
}

int yn_jpeg_scan_prepare(const uint8_t* data, int64_t len, uint8_t* unstuffed_host, int64_t cap, int32_t* segments_host, int64_t seg_cap, int32_t* info4)
{
    int32_t scratch[4];
    g_jpeg_reason.clear();
    return ynk::jpeg_scan_prepare(data, len, unstuffed_host, cap, segments_host, seg_cap, info4 ? info4 : scratch, g_jpeg_reason);
}

int yn_jpeg_entropy(yn_jpeg* j, int mode, int subseq_bits, int max_rounds)
{
    g_jpeg_reason.clear();
    if (!j) { g_jpeg_reason = "yn_jpeg_entropy: null object"; return 1; }
    return ynk::jpeg_entropy(j->st, mode, subseq_bits, max_rounds, g_jpeg_reason);
}

int yn_jpeg_entropy_stats(yn_jpeg* j, int64_t* device_files, int64_t* host_files, int32_t* rounds_last, int32_t* subseqs_last)
{
    if (!j) return 1;
    ynk::jpeg_entropy_stats(j->st, device_files, host_files, rounds_last, subseqs_last);
    return 0;
}

#define YN_JPEG_ENTER(name)                                                                                                               \
    YN_ENTER(h);                                                                                                                          \
    if (!j) return fail(h, name ": null object");                                                                                         \
    if (ynk::jpeg_device(j->st) != h->cfg.device)                                                                                         \
        return fail(h, name ": the object was made for device %d, the handle is on device %d", ynk::jpeg_device(j->st), h->cfg.device)

int yn_jpeg_device_coefficients(yn_handle* h, yn_jpeg* j, int i, int16_t* host, int64_t cap)
{
    YN_JPEG_ENTER("yn_jpeg_device_coefficients");
    YN_EVAL_CALL(ynk::jpeg_device_coefficients(j->st, h->stream, i, host, cap, err));
}

int yn_jpeg_entropy_states(yn_handle* h, yn_jpeg* j, int i, int32_t* host, int64_t cap)
{
    YN_JPEG_ENTER("yn_jpeg_entropy_states");
    YN_EVAL_CALL(ynk::jpeg_entropy_states(j->st, h->stream, i, host, cap, err));
}

int yn_jpeg_entropy_timing(yn_handle* h, yn_jpeg* j, float* ms7)
{
    YN_JPEG_ENTER("yn_jpeg_entropy_timing");
    if (!ms7) return fail(h, "yn_jpeg_entropy_timing: null argument");
    YN_EVAL_CALL(ynk::jpeg_entropy_timing(j->st, ms7, err));
}

// ---- baseline JPEG encode: every stage on the device (kernels_jpeg_enc.hip) ------------------------------------------------------------
int yn_jpeg_quant_tables(int quality, uint16_t* qt2x64_natural)
{
    if (!qt2x64_natural || quality < 1 || quality > 100) return 1;
    ynk::jpeg_quant_tables(quality, qt2x64_natural);
    return 0;
}

int yn_jpeg_header(int w, int h, int quality, int sampling, uint8_t* out623)
{
    if (!out623 || w < 1 || w > 16384 || h < 1 || h > 16384 || quality < 1 || quality > 100 || sampling < 0 || sampling > 2) return 1;
    ynk::jpeg_header(w, h, quality, sampling ? 2 : 1, sampling == 2 ? 2 : 1, out623);
    return 0;
}

int yn_jpeg_enc_create(yn_handle* h, int max_batch, int64_t stream_bytes, yn_jpeg_enc** out)
{
    YN_ENTER(h);
    if (!out) return fail(h, "yn_jpeg_enc_create: null argument");
    *out = nullptr;
    std::string err;
    ynk::JpegEncState* st = nullptr;
    if (ynk::jpeg_enc_create(h->cfg.device, max_batch, stream_bytes, &st, err)) return fail(h, "%s", err.c_str());
    *out = new yn_jpeg_enc{st};
    return 0;
}

void yn_jpeg_enc_destroy(yn_jpeg_enc* enc)
{
    if (!enc) return;
    ynk::jpeg_enc_destroy(enc->st);
    delete enc;
}

#define YN_JPEG_ENC_ENTER(name)                                                                                                           \
    YN_ENTER(h);                                                                                                                          \
    if (!enc) return fail(h, name ": null object");                                                                                       \
    if (ynk::jpeg_enc_device(enc->st) != h->cfg.device)                                                                                   \
        return fail(h, name ": the object was made for device %d, the handle is on device %d", ynk::jpeg_enc_device(enc->st), h->cfg.device)

int yn_jpeg_encode_batch(yn_handle* h, yn_jpeg_enc* enc, int n, const uint8_t* const* frames_host, const int32_t* geom_host, int quality, int sampling)
{
    YN_JPEG_ENC_ENTER("yn_jpeg_encode_batch");
    YN_EVAL_CALL(ynk::jpeg_encode_batch(enc->st, h->stream, n, frames_host, geom_host, quality, sampling, err));
}

int yn_jpeg_encode_fetch(yn_handle* h, yn_jpeg_enc* enc, int64_t* offsets_host, uint8_t* files_host, int64_t cap)
{
    YN_JPEG_ENC_ENTER("yn_jpeg_encode_fetch");
    YN_EVAL_CALL(ynk::jpeg_encode_fetch(enc->st, h->stream, offsets_host, files_host, cap, err));
}

int yn_jpeg_enc_coefficients(yn_handle* h, yn_jpeg_enc* enc, int i, int16_t* host, int64_t cap)
{
    YN_JPEG_ENC_ENTER("yn_jpeg_enc_coefficients");
    YN_EVAL_CALL(ynk::jpeg_enc_coefficients(enc->st, h->stream, i, host, cap, err));
}

int yn_jpeg_enc_guard(yn_handle* h, yn_jpeg_enc* enc, uint8_t* host64)
{
    YN_JPEG_ENC_ENTER("yn_jpeg_enc_guard");
    if (!host64) return fail(h, "yn_jpeg_enc_guard: null argument");
    YN_EVAL_CALL(ynk::jpeg_enc_guard(enc->st, h->stream, host64, err));
}

int yn_jpeg_enc_timing(yn_handle* h, yn_jpeg_enc* enc, float* ms10)
{
    YN_JPEG_ENC_ENTER("yn_jpeg_enc_timing");
    if (!ms10) return fail(h, "yn_jpeg_enc_timing: null argument");
    YN_EVAL_CALL(ynk::jpeg_enc_timing(enc->st, ms10, err));
}

}  // extern "C"
#pragma GCC visibility pop

// the training step, in dependency order: shared pieces, the two executors, the wiring they both run, the entry points
#include "yn_train_shared.inc"
#include "yn_train.inc"
#include "yn_train_h16.inc"
#include "yn_train_h16_ops.inc"
#include "yn_train_ops.inc"
#include "yn_train_tape.inc"
#include "yn_train_api.inc"
