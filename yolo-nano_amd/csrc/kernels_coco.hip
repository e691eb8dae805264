// kernels_coco.hip — COCO box AP as pycocotools' COCOeval computes it for iouType 'bbox' (computeIoU / bbIou, evaluateImg, accumulate)
// behind evaluator/cocoapi_evaluator.py:85-130, on the device.  Built with -ffp-contract=off: every double below is one operation of
// the published algorithm.  summarize (12 means over the two result arrays) stays on the host, in numpy, by design.
//
//   add      coco_ingest_kernel   yn_pack_detections records -> image pixels (:85-87, float32 steps), counted per (image, category)
//            coco_scan_kernel     exclusive offsets of the raw groups and of the groups cut to max_det
//            coco_scatter_kernel  record indices grouped by (image, category) (any order inside a group)
//            coco_rank_kernel     one wave per group: rank = number of records that go first (higher score; equal score and earlier
//                                 in the results list), which IS the stable sort by -score; ranks below max_det go to the store
//   finish   coco_match_kernel    one workgroup per (image, category), one wave per area range: ground truth across lanes, detections
//                                 walked in rank order, the greedy loop of evaluateImg replayed for every IoU threshold at once
//            coco_keys_kernel +   accumulate's order: 128-bit keys (category, -score | image in ascending id, rank, store index),
//            bitonic_sort         unique, so any correct sort gives the one stable order
//            coco_curve_kernel    one workgroup per (category, area range, maxDet): integer scans of tp / fp, float64 rc and pr,
//                                 precision at the recall thresholds, last recall
//
// All counts are integers (atomics on them are order-free); the only other atomic is an integer max on the bit pattern of a
// non-negative double, which is exact and order-free as well.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "yn_internal.h"
#include "yn_eval_shared.h"

namespace ynk {

namespace {

using namespace evs;

constexpr int CO_T = 10;                       // IoU thresholds at most (one matched and one ignored bit each in a 32-bit flag word)
constexpr int CO_A = 4;                        // area ranges at most: one wave of the match workgroup each
constexpr int CO_M = 8;                        // maxDets entries at most
constexpr int CO_R = 256;                      // recall thresholds at most
constexpr int CO_MAX_GT = 4096;                // GT per (image, category): 64 chunks of 64, one matched bit per chunk in each lane's mask
constexpr int CO_MAX_KEEP = 1023;              // max_det at most (10 bits of the sort key)
constexpr int CO_MAX_IMG = 1 << 21;
enum { CO_ERR_COORD = 1, CO_ERR_CLASS = 2, CO_ERR_SCORE = 4 };

struct CocoParams {
    double thr0[CO_T];                         // min(iouThr, 1 - 1e-10)
    double area[CO_A][2];
    int max_dets[CO_M];
};

struct Key128 { uint64_t hi, lo; };
__host__ __device__ __forceinline__ bool operator>(const Key128& a, const Key128& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
__host__ __device__ __forceinline__ bool operator<(const Key128& a, const Key128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// ---- add ----------------------------------------------------------------------------------------------------------------------
// tmp [total][5] = x1, y1, x2, y2 in image pixels (float32, as the reference's array holds them) and the score; pc [total] = b * C + category
__global__ void coco_ingest_kernel(const float* __restrict__ rec, const int32_t* __restrict__ offsets, int B,
                                   const int32_t* __restrict__ geom, int C, float* __restrict__ tmp, int32_t* __restrict__ pc,
                                   int32_t* __restrict__ cnt, int* err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= offsets[B]) return;
    const int b = image_of(offsets, B, i);
    const float* r = rec + 6 * i;
    float px[4];
    unletterbox(r, geom + 7 * b, px);
    int bits = 0;
    for (int c = 0; c < 4; ++c) {
        if (!(fabsf(px[c]) <= FLT_MAX)) bits |= CO_ERR_COORD;
        tmp[5 * i + c] = px[c];
    }
    const float sc = r[4];
    if (!(fabsf(sc) <= FLT_MAX)) bits |= CO_ERR_SCORE;
    tmp[5 * i + 4] = sc;
    const float cf = r[5];
    int cls = 0;
    if (cf >= 0.f && cf < (float)C && cf == floorf(cf)) cls = (int)cf; else bits |= CO_ERR_CLASS;
    if (bits) atomicOr(err, bits);
    const int p = b * C + cls;
    pc[i] = p;
    atomicAdd(&cnt[p], 1);
}

// start [P+1] / kstart [P+1]: exclusive sums of cnt and of min(cnt, keep); *kept = kstart[P]
__global__ __launch_bounds__(256) void coco_scan_kernel(const int32_t* __restrict__ cnt, int P, int keep, int32_t* __restrict__ start,
                                                        int32_t* __restrict__ kstart, int32_t* __restrict__ kept)
{
    __shared__ uint64_t lds[4];
    const int t = threadIdx.x;
    uint64_t carry = 0;                                          // raw << 32 | kept so far
    for (int base = 0; base < P; base += 256) {
        const int j = base + t;
        const uint32_t c = j < P ? (uint32_t)cnt[j] : 0u, k = c < (uint32_t)keep ? c : (uint32_t)keep;
        const uint64_t v = block_scan_incl((uint64_t)c << 32 | k, [](uint64_t x, uint64_t y) { return x + y; }, lds) + carry;
        if (j < P) {
            start[j] = (int32_t)((v >> 32) - c);
            kstart[j] = (int32_t)((v & 0xffffffffu) - k);
        }
        if (t == 255) lds[0] = v;
        __syncthreads();
        carry = lds[0];
        __syncthreads();
    }
    if (t == 0) {
        start[P] = (int32_t)(carry >> 32);
        kstart[P] = (int32_t)(carry & 0xffffffffu);
        *kept = kstart[P];
    }
}

__global__ void coco_scatter_kernel(const int32_t* __restrict__ pc, int total, const int32_t* __restrict__ start,
                                    int32_t* __restrict__ fill, int32_t* __restrict__ grp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int p = pc[i];
    grp[start[p] + atomicAdd(&fill[p], 1)] = i;
}

// One wave per (image, category) group p.  det [..][5] is the store, seg [P+1] this batch's slice of the segment table.
__global__ __launch_bounds__(256) void coco_rank_kernel(const float* __restrict__ tmp, const int32_t* __restrict__ grp,
                                                        const int32_t* __restrict__ start, const int32_t* __restrict__ kstart, int P,
                                                        int keep, int64_t n0, float* __restrict__ det, int64_t* __restrict__ seg)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int s = start[p], g = start[p + 1] - s;
    const int64_t o0 = n0 + kstart[p];
    if (lane == 0) {
        seg[p] = o0;
        if (p == P - 1) seg[P] = n0 + kstart[P];
    }
    for (int m = lane; m < g; m += 64) {
        const int i = grp[s + m];
        const float si = tmp[5 * i + 4];
        int rank = 0;
        for (int j = 0; j < g; ++j) {
            const int ij = grp[s + j];
            const float sj = tmp[5 * ij + 4];
            rank += (sj > si || (sj == si && ij < i)) ? 1 : 0;   // argsort(-score, kind='mergesort'): ties keep results-list order
        }
        if (rank < keep) {
            float* q = det + 5 * (o0 + rank);
            for (int c = 0; c < 5; ++c) q[c] = tmp[5 * i + c];
        }
    }
}

// ---- evaluateImg --------------------------------------------------------------------------------------------------------------
// Workgroup p = image (add order) * C + category; wave a = area range.  gt [G][5] = x, y, w, h, area grouped by (image, category) in
// file order, gt_seg [pairs + 1].  flags [A][n]: bit t = matched at threshold t, bit 16 + t = ignored at threshold t.
// The candidate order of the greedy loop (ground truth re-sorted with the non-ignored first, file order inside each group; a later
// box replaces an earlier one of equal IoU; ignored boxes only if no other matched) is the lexicographic maximum of
// (non-ignored, IoU, index) over the boxes still available with IoU >= min(t, 1 - 1e-10).
__global__ __launch_bounds__(256) void coco_match_kernel(const float* __restrict__ det, const int64_t* __restrict__ seg,
                                                         const double* __restrict__ gt, const uint8_t* __restrict__ gt_crowd,
                                                         const int32_t* __restrict__ gt_seg, int C, int T, int A, CocoParams prm,
                                                         uint32_t* __restrict__ flags, int64_t n, unsigned long long* __restrict__ npig)
{
    const int lane = threadIdx.x & 63, a = threadIdx.x >> 6;
    const int64_t p = blockIdx.x;
    if (a >= A) return;
    const int64_t d0 = seg[p];
    const int D = (int)(seg[p + 1] - d0);
    const int g0 = gt_seg[p], G = gt_seg[p + 1] - g0;
    if (D == 0 && G == 0) return;
    const int c = (int)(p % C);
    const double lo = prm.area[a][0], hi = prm.area[a][1];
    const int nch = (G + 63) >> 6;
    double r0x = 0, r0y = 0, r0w = 0, r0h = 0;                   // chunk 0 stays in registers
    bool r0ig = false, r0crowd = false;
    unsigned long long np = 0;
    for (int ch = 0; ch < nch; ++ch) {
        const int g = ch * 64 + lane;
        bool ig = true;
        if (g < G) {
            const double* q = gt + 5 * (int64_t)(g0 + g);
            const bool crowd = gt_crowd[g0 + g] != 0;
            ig = crowd || q[4] < lo || q[4] > hi;                // gtIg: the ANNOTATION area
            if (ch == 0) { r0x = q[0]; r0y = q[1]; r0w = q[2]; r0h = q[3]; r0ig = ig; r0crowd = crowd; }
        }
        np += __popcll(__ballot(!ig));
    }
    if (lane == 0 && np) atomicAdd(&npig[c * A + a], np);
    uint64_t claimed[CO_T];                                      // [t] bit ch: GT ch * 64 + lane is matched at threshold t
#pragma unroll
    for (int t = 0; t < CO_T; ++t) claimed[t] = 0;
    for (int d = 0; d < D; ++d) {
        const float* q = det + 5 * (d0 + d);
        const double dx = (double)q[0], dy = (double)q[1];
        const double dw = (double)q[2] - dx, dh = (double)q[3] - dy;   // bbox = [x1, y1, x2 - x1, y2 - y1] of the float() values
        const double da = dw * dh;
        int bcls[CO_T], bidx[CO_T];
        double biou[CO_T];
#pragma unroll
        for (int t = 0; t < CO_T; ++t) { bcls[t] = 0; bidx[t] = -1; biou[t] = 0.0; }
        for (int ch = 0; ch < nch; ++ch) {
            const int g = ch * 64 + lane;
            double gx = r0x, gy = r0y, gw = r0w, gh = r0h;
            bool ig = r0ig, crowd = r0crowd;
            if (ch > 0 && g < G) {
                const double* qg = gt + 5 * (int64_t)(g0 + g);
                gx = qg[0]; gy = qg[1]; gw = qg[2]; gh = qg[3];
                crowd = gt_crowd[g0 + g] != 0;
                ig = crowd || qg[4] < lo || qg[4] > hi;
            }
            double iou = 0.0;                                    // bbIou
            if (g < G) {
                const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
                if (w > 0) {
                    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
                    if (h > 0) {
                        const double in = w * h;
                        const double u = crowd ? da : (da + gw * gh) - in;
                        iou = in / u;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < CO_T; ++t) {
                if (t >= T) continue;
                const bool avail = g < G && (crowd || !((claimed[t] >> ch) & 1));
                const bool valid = avail && iou >= prm.thr0[t];
                if (!__any(valid)) continue;
                int cl = valid ? (ig ? 1 : 2) : 0, ix = g;
                double v = iou;
                for (int w = 32; w > 0; w >>= 1) {               // highest index among equal maxima, non-ignored before ignored
                    const int cl2 = __shfl_xor(cl, w), ix2 = __shfl_xor(ix, w);
                    const double v2 = __shfl_xor(v, w);
                    if (cl2 > cl || (cl2 == cl && (v2 > v || (v2 == v && ix2 > ix)))) { cl = cl2; v = v2; ix = ix2; }
                }
                if (cl > bcls[t] || (cl == bcls[t] && v >= biou[t])) { bcls[t] = cl; biou[t] = v; bidx[t] = ix; }
            }
        }
        const bool out = da < lo || da > hi;                     // an unmatched detection is ignored by ITS area w * h
        uint32_t word = 0;
#pragma unroll
        for (int t = 0; t < CO_T; ++t) {
            if (t >= T) continue;
            if (bcls[t] > 0) {
                word |= 1u << t;
                if (bcls[t] == 1) word |= 1u << (16 + t);
                if (lane == (bidx[t] & 63)) claimed[t] |= 1ull << (bidx[t] >> 6);
            } else if (out) {
                word |= 1u << (16 + t);
            }
        }
        if (lane == 0) flags[(int64_t)a * n + d0 + d] = word;
    }
}

// ---- accumulate ---------------------------------------------------------------------------------------------------------------
// key of store index i: hi = category << 32 | descending-score bits; lo = image in ascending id << 43 | rank << 33 | i
__global__ void coco_keys_kernel(const float* __restrict__ det, const int64_t* __restrict__ seg, int64_t P, int C,
                                 const int32_t* __restrict__ img_rank, int64_t n, int64_t npow, Key128* __restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npow) return;
    if (i >= n) { keys[i] = Key128{~0ull, ~0ull}; return; }      // padding sorts last (no real key has the top bits set)
    int64_t lo = 0, hi = P;                                      // the group p with seg[p] <= i < seg[p + 1]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t img = lo / C, c = lo % C, rank = i - seg[lo];
    float s = det[5 * i + 4];
    if (s == 0.f) s = 0.f;                                       // -0.0 == 0.0 for the sort
    const uint32_t u = __float_as_uint(s);
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    keys[i] = Key128{(uint64_t)c << 32 | (uint32_t)~asc, (uint64_t)img_rank[img] << 43 | (uint64_t)rank << 33 | (uint64_t)i};
}

// Workgroup (category c, area range a, maxDet m).  precision [T][R][C][A][M], recall [T][C][A][M].
// precision[t, r] = max of pr over the positions whose recall reaches recThrs[r] (the backward maximum read at searchsorted's
// index), and since pr only falls while tp stands still, that maximum is taken at true positives: each true positive offers its pr to
// the last threshold its recall reaches, and a suffix maximum over the thresholds finishes the row.
__global__ __launch_bounds__(256) void coco_curve_kernel(const Key128* __restrict__ keys, int64_t n, const uint32_t* __restrict__ flags,
                                                         const unsigned long long* __restrict__ npig, const double* __restrict__ rec_thrs,
                                                         CocoParams prm, int T, int R, int C, int A, int M,
                                                         double* __restrict__ precision, double* __restrict__ recall)
{
    __shared__ unsigned long long best[CO_T][CO_R];
    __shared__ double thr[CO_R];
    __shared__ uint64_t lds[4];
    const int c = blockIdx.x, a = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const unsigned long long np = npig[c * A + a];
    if (np == 0) {                                               // no non-ignored ground truth: both stay -1
        for (int j = tid; j < T * R; j += 256) precision[(((int64_t)j * C + c) * A + a) * M + m] = -1.0;
        if (tid < T) recall[(((int64_t)tid * C + c) * A + a) * M + m] = -1.0;
        return;
    }
    for (int j = tid; j < CO_T * CO_R; j += 256) best[j / CO_R][j % CO_R] = 0ull;
    for (int j = tid; j < R; j += 256) thr[j] = rec_thrs[j];
    __syncthreads();
    const int max_det = prm.max_dets[m];
    const int64_t s = lower_bound(keys, n, Key128{(uint64_t)c << 32, 0ull}), e = lower_bound(keys, n, Key128{(uint64_t)(c + 1) << 32, 0ull});
    const double npd = (double)np;
    uint64_t carry[CO_T];                                        // tp << 32 | fp so far
#pragma unroll
    for (int t = 0; t < CO_T; ++t) carry[t] = 0;
    for (int64_t base = s; base < e; base += 256) {
        const int64_t pidx = base + tid;
        bool in = false;
        uint32_t word = 0;
        if (pidx < e) {
            const uint64_t l = keys[pidx].lo;
            in = (int)((l >> 33) & 1023) < max_det;              // the first maxDet detections of each image
            word = flags[(int64_t)a * n + (int64_t)(l & ((1ull << 33) - 1))];
        }
#pragma unroll
        for (int t = 0; t < CO_T; ++t) {
            if (t >= T) continue;
            const bool mt = (word >> t) & 1, ig = (word >> (16 + t)) & 1;
            const bool tp = in && mt && !ig, fp = in && !mt && !ig;
            const uint64_t v = block_scan_incl((uint64_t)tp << 32 | (uint64_t)fp, [](uint64_t x, uint64_t y) { return x + y; }, lds) + carry[t];
            if (tp) {
                const double tpd = (double)(v >> 32), fpd = (double)(v & 0xffffffffu);
                const double rc = tpd / npd;
                const double pr = tpd / ((fpd + tpd) + DBL_EPSILON);     // np.spacing(1)
                int lo = 0, hi = R;                              // number of thresholds <= rc
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (thr[mid] <= rc) lo = mid + 1; else hi = mid;
                }
                if (lo > 0) atomicMax(&best[t][lo - 1], (unsigned long long)__double_as_longlong(pr));
            }
            if (tid == 255) lds[0] = v;
            __syncthreads();
            carry[t] = lds[0];
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < T) {
        uint64_t c_t = 0;
#pragma unroll
        for (int t = 0; t < CO_T; ++t) if (t == tid) c_t = carry[t];
        recall[(((int64_t)tid * C + c) * A + a) * M + m] = (double)(c_t >> 32) / npd;   // rc[-1], 0 without detections
        unsigned long long run = 0;                              // non-negative doubles order as their bit patterns
        for (int r = R - 1; r >= 0; --r) {
            const unsigned long long b = best[tid][r];
            run = b > run ? b : run;
            precision[((((int64_t)tid * R + r) * C + c) * A + a) * M + m] = __longlong_as_double((long long)run);
        }
    }
}

}  // namespace

// ---- state ----------------------------------------------------------------------------------------------------------------------
struct CocoState {
    int device = 0, C = 0, keep = 100;
    int64_t n = 0;                             // detections in the store
    int n_img = 0;
    DevBuf<float> det;                         // [cap / 5][5]
    DevBuf<int64_t> seg;                       // [n_img * C + 1]
    // per-add scratch
    DevBuf<float> tmp;
    DevBuf<int32_t> pc, grp, cnt, fill, start, kstart, geom_dev, kept_dev;
    PinnedBuf<int32_t> pinned;
    DevBuf<int> err_dev;
    // ground truth (host until finish), grouped by (image, category), file order inside
    std::vector<int64_t> ids;
    std::vector<double> gt;                    // [G][5] x, y, w, h, area
    std::vector<uint8_t> gt_crowd;
    std::vector<int32_t> gt_seg{0};            // [n_img * C + 1]
    // finish
    DevBuf<double> gt_dev;
    DevBuf<uint8_t> crowd_dev;
    DevBuf<int32_t> gt_seg_dev, rank_dev;
    DevBuf<uint32_t> flags;
    DevBuf<Key128> keys;
    DevBuf<unsigned long long> npig;
    DevBuf<double> rec_thrs, prec_dev, recall_dev;
    bool finished = false;
    int fin_A = 0;
};

namespace {

const char* coco_err_text(int bits)
{
    if (bits & CO_ERR_CLASS) return "a detection category is not an integer in 0..C-1";
    if (bits & CO_ERR_COORD) return "a detection coordinate in pixels is not finite";
    return "a detection score is not finite";
}

}  // namespace

int coco_create(int device, int C, int max_det, CocoState** out, std::string& err)
{
    if (C < 1 || C > 2000) { err = "yn_coco_create: num_classes must be 1..2000"; return 1; }
    if (max_det < 1 || max_det > CO_MAX_KEEP) { err = "yn_coco_create: max_det must be 1..1023"; return 1; }
    auto* e = new CocoState;
    e->device = device; e->C = C; e->keep = max_det;
    int r = e->err_dev.reserve(4);
    if (!r) r = e->kept_dev.reserve(4);
    if (!r) r = e->pinned.reserve(64);
    if (!r) r = hipMemset(e->err_dev, 0, 16);
    if (r) { err = std::string("yn_coco_create: ") + hipGetErrorString((hipError_t)r); coco_destroy(e); return 1; }
    *out = e;
    return 0;
}

void coco_destroy(CocoState* e)
{
    if (!e) return;
    DeviceScope on(e->device);
    delete e;
}

int coco_reset(CocoState* e, hipStream_t s, std::string& err)
{
    EVCHK(hipStreamSynchronize(s));
    e->n = 0; e->n_img = 0;
    e->ids.clear(); e->gt.clear(); e->gt_crowd.clear(); e->gt_seg.assign(1, 0);
    e->finished = false;
    EVCHK(hipMemsetAsync(e->err_dev, 0, 16, s));
    return 0;
}

// 0 ok, 1 error, 2 range mark (offsets[B] < 0): nothing added
int coco_add(CocoState* e, hipStream_t s, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom,
             const int64_t* image_ids, const double* gt, const int32_t* gt_meta, const int32_t* gt_off, std::string& err)
{
    if (B <= 0 || !rec_dev || !offsets_dev || !geom || !image_ids || !gt_off) { err = "yn_coco_add: bad arguments"; return 1; }
    if (gt_off[0] != 0) { err = "yn_coco_add: gt_offsets[0] must be 0"; return 1; }
    const int C = e->C;
    if ((int64_t)B * C >= (1 << 30)) { err = "yn_coco_add: batch too large"; return 1; }
    for (int b = 0; b < B; ++b) {
        if (gt_off[b + 1] < gt_off[b]) { err = "yn_coco_add: gt_offsets must not decrease"; return 1; }
        const int32_t* g = geom + 7 * b;
        if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0 || g[6] <= 0) { err = "yn_coco_add: geometry needs positive w0, h0, rw, rh, side"; return 1; }
    }
    if (gt_off[B] > 0 && (!gt || !gt_meta)) { err = "yn_coco_add: ground truth pointer is null"; return 1; }
    if ((int64_t)e->n_img + B >= CO_MAX_IMG) { err = "yn_coco_add: more than 2^21 images"; return 1; }
    if ((int64_t)e->gt_crowd.size() + gt_off[B] >= ((int64_t)1 << 31)) { err = "yn_coco_add: more than 2^31 - 1 ground-truth boxes"; return 1; }
    // the ground truth first (host only): validated before anything is changed
    std::vector<int> cnt(C);
    for (int b = 0; b < B; ++b) {
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int i = gt_off[b]; i < gt_off[b + 1]; ++i) {
            const int cat = gt_meta[2 * (int64_t)i];
            if (cat < 0 || cat >= C) { err = "yn_coco_add: ground-truth category out of range"; return 1; }
            for (int k = 0; k < 5; ++k)
                if (!std::isfinite(gt[5 * (int64_t)i + k])) { err = "yn_coco_add: ground-truth box or area is not finite"; return 1; }
            if (++cnt[cat] > CO_MAX_GT) { err = "yn_coco_add: more than 4096 ground-truth boxes of one category in one image"; return 1; }
        }
    }
    if (e->pinned.cap() < 1 + 7 * (size_t)B) {
        EVCHK(hipStreamSynchronize(s));
        EVCHK(e->pinned.reserve(1 + 7 * (size_t)B));
    }
    EVCHK(hipMemcpyAsync(e->pinned, offsets_dev + B, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));            // also retires the previous batch's use of the staging and scratch buffers
    const int32_t total = e->pinned[0];
    if (total < 0) { err = "yn_coco_add: offsets[B] is negative (split-f16 range mark): nothing added"; return 2; }
    if (e->n + total >= ((int64_t)1 << 31)) { err = "yn_coco_add: more than 2^31 - 1 detections"; return 1; }
    const int P = B * C;
    const size_t tn = total > 0 ? (size_t)total : 1;
    EVCHK(e->tmp.reserve(5 * tn, 1));              // every scratch buffer doubles from one element
    EVCHK(e->pc.reserve(tn, 1));
    EVCHK(e->grp.reserve(tn, 1));
    EVCHK(e->cnt.reserve((size_t)P, 1));
    EVCHK(e->fill.reserve((size_t)P, 1));
    EVCHK(e->start.reserve((size_t)P + 1, 1));
    EVCHK(e->kstart.reserve((size_t)P + 1, 1));
    EVCHK(e->geom_dev.reserve(7 * (size_t)B, 1));
    memcpy(e->pinned + 1, geom, 7 * (size_t)B * sizeof(int32_t));
    EVCHK(hipMemcpyAsync(e->geom_dev, e->pinned + 1, 7 * (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EVCHK(hipMemsetAsync(e->cnt, 0, (size_t)P * sizeof(int32_t), s));
    EVCHK(hipMemsetAsync(e->fill, 0, (size_t)P * sizeof(int32_t), s));
    if (total > 0)
        hipLaunchKernelGGL(coco_ingest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rec_dev, offsets_dev, B,
                           (const int32_t*)e->geom_dev, C, e->tmp, e->pc, e->cnt, e->err_dev);
    hipLaunchKernelGGL(coco_scan_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)e->cnt, P, e->keep, e->start, e->kstart, e->kept_dev);
    EVCHK(hipGetLastError());
    EVCHK(hipMemcpyAsync(e->pinned, e->kept_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    const int32_t kept = e->pinned[0];
    if (kept < 0 || kept > total) { err = "yn_coco_add: internal count mismatch"; return 1; }
    EVCHK(e->det.reserve_keep(5 * (size_t)(e->n + kept) + 5, 5 * (size_t)e->n, s, 4096));
    EVCHK(e->seg.reserve_keep((size_t)(e->n_img + B) * C + 1, e->n_img ? (size_t)e->n_img * C + 1 : 0, s, 4096));
    if (total > 0)
        hipLaunchKernelGGL(coco_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const int32_t*)e->pc, (int)total,
                           (const int32_t*)e->start, e->fill, e->grp);
    hipLaunchKernelGGL(coco_rank_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, (const float*)e->tmp, (const int32_t*)e->grp,
                       (const int32_t*)e->start, (const int32_t*)e->kstart, P, e->keep, e->n, e->det, e->seg + (size_t)e->n_img * C);
    EVCHK(hipGetLastError());
    // ground truth: per image, grouped by category in file order
    std::vector<std::vector<int>> by_cat(C);
    for (int b = 0; b < B; ++b) {
        for (auto& v : by_cat) v.clear();
        for (int i = gt_off[b]; i < gt_off[b + 1]; ++i) by_cat[gt_meta[2 * (int64_t)i]].push_back(i);
        for (int c = 0; c < C; ++c) {
            for (int i : by_cat[c]) {
                e->gt.insert(e->gt.end(), gt + 5 * (int64_t)i, gt + 5 * (int64_t)i + 5);
                e->gt_crowd.push_back(gt_meta[2 * (int64_t)i + 1] ? 1 : 0);
            }
            e->gt_seg.push_back((int32_t)e->gt_crowd.size());
        }
        e->ids.push_back(image_ids[b]);
    }
    e->n += kept;
    e->n_img += B;
    e->finished = false;
    EVCHK(hipStreamSynchronize(s));            // the next add or the finish may come on another handle's stream
    return 0;
}

int coco_finish(CocoState* e, hipStream_t s, const double* iou_thrs, int T, const double* rec_thrs, int R, const double* area_rng, int A,
                const int32_t* max_dets, int M, double* precision_host, double* recall_host, std::string& err)
{
    if (!iou_thrs || !rec_thrs || !area_rng || !max_dets || !precision_host || !recall_host) { err = "yn_coco_finish: null argument"; return 1; }
    if (T < 1 || T > CO_T || R < 1 || R > CO_R || A < 1 || A > CO_A || M < 1 || M > CO_M) {
        err = "yn_coco_finish: at most 10 IoU thresholds, 256 recall thresholds, 4 area ranges and 8 maxDets"; return 1;
    }
    CocoParams prm{};
    for (int t = 0; t < T; ++t) {
        if (!(iou_thrs[t] == iou_thrs[t])) { err = "yn_coco_finish: an IoU threshold is NaN"; return 1; }
        prm.thr0[t] = std::min(iou_thrs[t], 1 - 1e-10);
    }
    for (int r = 0; r < R; ++r)
        if (!(rec_thrs[r] == rec_thrs[r]) || (r > 0 && rec_thrs[r] < rec_thrs[r - 1])) { err = "yn_coco_finish: recall thresholds must ascend"; return 1; }
    for (int a = 0; a < A; ++a) { prm.area[a][0] = area_rng[2 * a]; prm.area[a][1] = area_rng[2 * a + 1]; }
    for (int m = 0; m < M; ++m) {
        if (max_dets[m] < 1 || (m > 0 && max_dets[m] < max_dets[m - 1])) { err = "yn_coco_finish: maxDets must be positive and ascend"; return 1; }
        prm.max_dets[m] = max_dets[m];
    }
    if (max_dets[M - 1] != e->keep) { err = "yn_coco_finish: the last maxDets entry must be the max_det given to yn_coco_create"; return 1; }
    const int C = e->C, n_img = e->n_img;
    const int64_t n = e->n, P = (int64_t)n_img * C;
    // images in ascending id: COCOeval walks sorted(unique(imgIds)), and that decides ties between images
    std::vector<int32_t> order(n_img), rank(n_img);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return e->ids[x] < e->ids[y]; });
    for (int r = 0; r < n_img; ++r) {
        if (r > 0 && e->ids[order[r]] == e->ids[order[r - 1]]) { err = "yn_coco_finish: an image id was added twice"; return 1; }
        rank[order[r]] = r;
    }
    int64_t npow = SORT_LOCAL;
    while (npow < n) npow *= 2;
    const size_t np_out = (size_t)T * R * C * A * M, nr_out = (size_t)T * C * A * M;
    EVCHK(hipStreamSynchronize(s));
    EVCHK(e->gt_dev.reserve(e->gt.size() + 5, 1));
    EVCHK(e->crowd_dev.reserve(e->gt_crowd.size() + 1, 1));
    EVCHK(e->gt_seg_dev.reserve(e->gt_seg.size(), 1));
    EVCHK(e->rank_dev.reserve((size_t)n_img + 1, 1));
    EVCHK(e->flags.reserve((size_t)A * (size_t)n + 1, 1));
    EVCHK(e->keys.reserve((size_t)npow, 1));
    EVCHK(e->npig.reserve((size_t)C * A, 1));
    EVCHK(e->rec_thrs.reserve((size_t)R, 1));
    EVCHK(e->prec_dev.reserve(np_out, 1));
    EVCHK(e->recall_dev.reserve(nr_out, 1));
    if (!e->gt.empty()) {
        EVCHK(hipMemcpyAsync(e->gt_dev, e->gt.data(), e->gt.size() * sizeof(double), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e->crowd_dev, e->gt_crowd.data(), e->gt_crowd.size(), hipMemcpyHostToDevice, s));
    }
    EVCHK(hipMemcpyAsync(e->gt_seg_dev, e->gt_seg.data(), e->gt_seg.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_img) EVCHK(hipMemcpyAsync(e->rank_dev, rank.data(), (size_t)n_img * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EVCHK(hipMemcpyAsync(e->rec_thrs, rec_thrs, (size_t)R * sizeof(double), hipMemcpyHostToDevice, s));
    EVCHK(hipMemsetAsync(e->npig, 0, (size_t)C * A * sizeof(unsigned long long), s));
    if (P > 0) {
        hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)P), dim3(256), 0, s, (const float*)e->det, (const int64_t*)e->seg,
                           (const double*)e->gt_dev, (const uint8_t*)e->crowd_dev, (const int32_t*)e->gt_seg_dev, C, T, A, prm, e->flags, n,
                           e->npig);
    }
    hipLaunchKernelGGL(coco_keys_kernel, dim3((unsigned)((npow + 255) / 256)), dim3(256), 0, s, (const float*)e->det, (const int64_t*)e->seg,
                       P, C, (const int32_t*)e->rank_dev, n, npow, e->keys);
    if (n > 0) bitonic_sort(e->keys.get(), npow, s);
    hipLaunchKernelGGL(coco_curve_kernel, dim3(C, A, M), dim3(256), 0, s, (const Key128*)e->keys, n, (const uint32_t*)e->flags,
                       (const unsigned long long*)e->npig, (const double*)e->rec_thrs, prm, T, R, C, A, M, e->prec_dev, e->recall_dev);
    EVCHK(hipGetLastError());
    int bits = 0;
    EVCHK(hipMemcpyAsync(precision_host, e->prec_dev, np_out * sizeof(double), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(recall_host, e->recall_dev, nr_out * sizeof(double), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(&bits, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    if (bits) { err = std::string("yn_coco_finish: ") + coco_err_text(bits); return 1; }
    e->finished = true;
    e->fin_A = A;
    return 0;
}

int coco_matches(CocoState* e, hipStream_t s, float* det_host, int64_t* seg_host, uint32_t* flags_host, int areas, std::string& err)
{
    if (!e->finished) { err = "yn_coco_matches: call yn_coco_finish first"; return 1; }
    if (areas != e->fin_A) { err = "yn_coco_matches: areas must be the count given to yn_coco_finish"; return 1; }
    if (e->n > 0) {
        if (det_host) EVCHK(hipMemcpyAsync(det_host, e->det, (size_t)e->n * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (flags_host) EVCHK(hipMemcpyAsync(flags_host, e->flags, (size_t)areas * (size_t)e->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    if (seg_host) {
        if (e->n_img) EVCHK(hipMemcpyAsync(seg_host, e->seg, ((size_t)e->n_img * e->C + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        else seg_host[0] = 0;
    }
    EVCHK(hipStreamSynchronize(s));
    return 0;
}

void coco_size(const CocoState* e, int64_t* detections, int64_t* images)
{
    if (detections) *detections = e->n;
    if (images) *images = e->n_img;
}

}  // namespace ynk
