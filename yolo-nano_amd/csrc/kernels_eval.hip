// kernels_eval.hip — the PASCAL VOC metric of evaluator/vocapi_evaluator.py (VOCAPIEvaluator.evaluate + do_python_eval + voc_eval +
// voc_ap) on the device, bit for bit.  Built with -ffp-contract=off: every double below is the reference's numpy operation sequence.
//
//   ingest   (eval_ingest_kernel)  yn_pack_detections records -> image pixels (:72-74, f32 steps) -> the text-file route (:154, :278-281)
//            as integers: score bin k = rint(s*1000) in 0..1000, coordinates in tenths rint(f32(b + 1)*10).  SoA, ingest order.
//   order    two bitonic sorts of UNIQUE 64-bit keys (the ingest index is part of each key, so any correct sort gives one order):
//            A = (class, 1000 - k, ingest index)         the per-class detection order of the PR curve (:284), ties in file order
//            B = (class, image, 1000 - k, index in image) the same order cut into (image, class) segments for the greedy match
//   match    (eval_match_kernel) one wave per (class, image): GT in registers (chunks of 64), detections walked in order, IoU across
//            lanes in double, cross-lane max / first argmax, NaN -> FP (:293-327).  Writes tp / fp / neither per ingest index.
//   curve    (eval_curve_kernel) one workgroup per class: cumulative tp / fp -> rec, prec (:328-333), suffix-max envelope, then the
//            11-point AP or the area AP with numpy's pairwise summation order (voc_ap :199-230).
//
// The reference's np.argsort (:284) is not stable, so its order among EQUAL 3-decimal scores depends on the numpy build; ours is the
// file order (image in add order, then position in that image's record list).  That is the one point where the reference is not
// deterministic; everything else is its arithmetic.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "yn_internal.h"
#include "yn_eval_shared.h"

namespace ynk {

namespace {

using namespace evs;                           // unletterbox, bitonic_sort, lower_bound, block_scan_incl, EVCHK, grow

constexpr int EV_LOCAL = SORT_LOCAL;           // keys per workgroup in the LDS stages of the bitonic sort
constexpr int EV_MAX_GT = 4096;                // GT per (image, class): 64 chunks of 64, one claimed bit per chunk in each lane's mask
constexpr uint64_t KEY_IDX_BITS = 43;          // key A: class 11 | 1000-k 10 | ingest index 43
constexpr uint64_t KEY_LOCAL_BITS = 22;        // key B: class 11 | image 21 | 1000-k 10 | index in image 22
enum { EV_ERR_SCORE = 1, EV_ERR_CLASS = 2, EV_ERR_COORD = 4, EV_ERR_IMAGE = 8 };

// ---- ingest ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tenths(float v, int* err)
{
    const double t = rint((double)v * 10.0);   // '{:.1f}'.format(v): v*10 is exact in double for a float32 v, ties to even as the formatter
    if (!(t > -2147483000.0 && t < 2147483000.0)) { atomicOr(err, EV_ERR_COORD); return 0; }
    return (int)t;
}

__global__ void eval_ingest_kernel(const float* __restrict__ rec, const int32_t* __restrict__ offsets, int B,
                                   const int32_t* __restrict__ geom, int C, int64_t n0, int img0,
                                   int32_t* __restrict__ soa, int64_t cap, int32_t* __restrict__ img_first, int* err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int total = offsets[B];
    if (i < B) {
        img_first[img0 + i] = (int32_t)(n0 + offsets[i]);
        if (offsets[i + 1] - offsets[i] >= (1 << KEY_LOCAL_BITS)) atomicOr(err, EV_ERR_IMAGE);
    }
    if (i >= total) return;
    const int b = image_of(offsets, B, i);
    const float* r = rec + 6 * i;
    const int64_t o = n0 + i;
    int32_t* out = soa;
    float px[4];
    unletterbox(r, geom + 7 * b, px);           // bboxes -= offset; bboxes /= scale; bboxes *= size  (float32 array, float64 operands)
    for (int c = 0; c < 4; ++c) out[(3 + c) * cap + o] = tenths(px[c] + 1.0f, err);   // dets[k, c] + 1: a float32 addition (NEP 50)
    const double ks = rint((double)r[4] * 1000.0);         // '{:.3f}'.format(score)
    int k = 0;
    if (ks >= 0.0 && ks <= 1000.0) k = (int)ks; else atomicOr(err, EV_ERR_SCORE);
    const float cf = r[5];
    int cls = 0;
    if (cf >= 0.f && cf < (float)C && cf == floorf(cf)) cls = (int)cf; else atomicOr(err, EV_ERR_CLASS);
    out[0 * cap + o] = img0 + b;
    out[1 * cap + o] = cls;
    out[2 * cap + o] = k;
}

__global__ void eval_keys_kernel(const int32_t* __restrict__ soa, int64_t cap, const int32_t* __restrict__ img_first, int64_t n,
                                 int64_t npow, uint64_t* __restrict__ keyA, uint64_t* __restrict__ keyB)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npow) return;
    if (i >= n) { keyA[i] = ~0ull; keyB[i] = ~0ull; return; }   // padding sorts last (no real key is all ones: C <= 2000)
    const uint64_t img = (uint32_t)soa[i], cls = (uint32_t)soa[cap + i], inv = 1000u - (uint32_t)soa[2 * cap + i];
    keyA[i] = (cls << 53) | (inv << KEY_IDX_BITS) | (uint64_t)i;
    keyB[i] = (cls << 53) | (img << 32) | (inv << KEY_LOCAL_BITS) | (uint64_t)(i - img_first[img]);
}

// ---- greedy match (:293-327) ----------------------------------------------------------------------------------------------------
// One wave per (class, image) pair, pair = c * n_img + img (the order of key B).  gt [G][5] = x1, y1, x2, y2, difficult grouped by
// (image, class) in file order, gt_seg [n_img * C + 1].  flag[ingest index] = 1 TP, 2 FP, 0 neither (difficult).
__global__ __launch_bounds__(256) void eval_match_kernel(const uint64_t* __restrict__ keyB, int64_t n, const int32_t* __restrict__ soa,
                                                         int64_t cap, const int32_t* __restrict__ img_first,
                                                         const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_seg,
                                                         int n_img, int C, double ovthresh, uint8_t* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (int64_t)n_img * C) return;
    const int c = (int)(pair / n_img), img = (int)(pair % n_img);
    const uint64_t prefix = ((uint64_t)c << 21 | (uint64_t)img);
    const int64_t lo = lower_bound(keyB, n, prefix << 32), hi = lower_bound(keyB, n, (prefix + 1) << 32);
    if (lo >= hi) return;
    const int g0 = gt_seg[(int64_t)img * C + c], G = gt_seg[(int64_t)img * C + c + 1] - g0;
    const int nch = (G + 63) >> 6;
    double r0x1 = 0, r0y1 = 0, r0x2 = 0, r0y2 = 0;               // chunk 0 stays in registers (VOC: a handful of GT per image)
    if (lane < G) {
        const int32_t* q = gt + 5 * (g0 + lane);
        r0x1 = q[0]; r0y1 = q[1]; r0x2 = q[2]; r0y2 = q[3];
    }
    uint64_t claimed = 0;                                        // bit ch: GT ch*64 + lane already detected (R['det'])
    const int32_t first = img_first[img];
    for (int64_t d0 = lo; d0 < hi; d0 += 64) {
        const int nd = (int)(hi - d0 < 64 ? hi - d0 : 64);
        int64_t my_idx = 0;
        double mx1 = 0, my1 = 0, mx2 = 0, my2 = 0;
        if (lane < nd) {
            my_idx = first + (int64_t)(keyB[d0 + lane] & ((1ull << KEY_LOCAL_BITS) - 1));
            mx1 = soa[3 * cap + my_idx] / 10.0;                 // float('%.1f'): the tenths back as the nearest double
            my1 = soa[4 * cap + my_idx] / 10.0;
            mx2 = soa[5 * cap + my_idx] / 10.0;
            my2 = soa[6 * cap + my_idx] / 10.0;
        }
        uint8_t my_res = 2;
        for (int d = 0; d < nd; ++d) {
            const double bx1 = __shfl(mx1, d), by1 = __shfl(my1, d), bx2 = __shfl(mx2, d), by2 = __shfl(my2, d);
            const double barea = (bx2 - bx1) * (by2 - by1);
            double best = -INFINITY;
            int bidx = -1;
            bool any_nan = false;
            for (int ch = 0; ch < nch; ++ch) {
                const int g = ch * 64 + lane;
                double gx1 = r0x1, gy1 = r0y1, gx2 = r0x2, gy2 = r0y2;
                if (ch > 0 && g < G) {
                    const int32_t* q = gt + 5 * (g0 + g);
                    gx1 = q[0]; gy1 = q[1]; gx2 = q[2]; gy2 = q[3];
                }
                double ov = -INFINITY;
                int oi = 0x7fffffff;
                if (g < G) {
                    const double ixmin = fmax(gx1, bx1), iymin = fmax(gy1, by1);     // np.maximum / np.minimum: no NaN among coordinates
                    const double ixmax = fmin(gx2, bx2), iymax = fmin(gy2, by2);
                    const double iw = fmax(ixmax - ixmin, 0.0), ih = fmax(iymax - iymin, 0.0);
                    const double inters = iw * ih;
                    const double uni = (barea + (gx2 - gx1) * (gy2 - gy1)) - inters;
                    ov = inters / uni;
                    oi = g;
                }
                any_nan |= __any(ov != ov) != 0;
                for (int w = 32; w > 0; w >>= 1) {               // max, first index among equals (np.max / np.argmax)
                    const double ov2 = __shfl_xor(ov, w);
                    const int oi2 = __shfl_xor(oi, w);
                    if (ov2 > ov || (ov2 == ov && oi2 < oi)) { ov = ov2; oi = oi2; }
                }
                if (ov > best || bidx < 0) { best = ov; bidx = oi; }
            }
            uint8_t res = 2;                                     // FP unless a match
            if (!any_nan && G > 0 && best > ovthresh) {
                if (gt[5 * (g0 + bidx) + 4]) {
                    res = 0;                                     // difficult: neither TP nor FP
                } else {
                    const uint64_t m = __shfl(claimed, bidx & 63);
                    if ((m >> (bidx >> 6)) & 1) {
                        res = 2;
                    } else {
                        res = 1;
                        if (lane == (bidx & 63)) claimed |= 1ull << (bidx >> 6);
                    }
                }
            }
            if (lane == d) my_res = res;
        }
        if (lane < nd) flag[my_idx] = my_res;
    }
}

// ---- PR curve + AP (:328-333, voc_ap :199-230) ----------------------------------------------------------------------------------
constexpr int CT = 256;                                          // threads of eval_curve_kernel

// numpy's pairwise_sum of float64 (n <= 128: eight accumulators; longer: split at n/2 rounded down to a multiple of 8), as an
// explicit post-order walk.
__device__ double pairwise_sum(const double* a, int64_t n)
{
    int64_t st_off[64], st_n[64];
    double vals[64];
    int sp = 0, vp = 0;
    st_off[0] = 0; st_n[0] = n; sp = 1;
    while (sp > 0) {
        --sp;
        const int64_t off = st_off[sp], m = st_n[sp];
        if (m < 0) {                                             // combine marker
            const double r = vals[--vp], l = vals[--vp];
            vals[vp++] = l + r;
            continue;
        }
        if (m <= 128) {
            const double* p = a + off;
            double res;
            if (m < 8) {
                res = 0.0;
                for (int64_t i = 0; i < m; ++i) res += p[i];
            } else {
                double r[8];
                for (int j = 0; j < 8; ++j) r[j] = p[j];
                int64_t i = 8;
                for (; i < m - (m % 8); i += 8)
                    for (int j = 0; j < 8; ++j) r[j] += p[i + j];
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < m; ++i) res += p[i];
            }
            vals[vp++] = res;
            continue;
        }
        int64_t n2 = m / 2;
        n2 -= n2 % 8;
        st_off[sp] = 0; st_n[sp] = -1; ++sp;                     // after both halves: add
        st_off[sp] = off + n2; st_n[sp] = m - n2; ++sp;          // right, evaluated second
        st_off[sp] = off; st_n[sp] = n2; ++sp;                   // left, evaluated first
    }
    return vals[0];
}

__device__ double numpy_sum(const double* a, int64_t n)          // np.sum of a contiguous float64 vector: 0.0 + pairwise per 8192 block
{
    double res = 0.0;
    for (int64_t s = 0; s < n; s += 8192) res += pairwise_sum(a + s, n - s < 8192 ? n - s : 8192);
    return res;
}

__global__ __launch_bounds__(CT) void eval_curve_kernel(const uint64_t* __restrict__ keyA, int64_t n, const uint8_t* __restrict__ flag,
                                                        const int64_t* __restrict__ npos, int use07, double* __restrict__ rec,
                                                        double* __restrict__ prec, double* __restrict__ env, int32_t* __restrict__ pts,
                                                        double* __restrict__ terms, double* __restrict__ ap, int64_t* __restrict__ cls_start)
{
    __shared__ uint64_t lds_u[4];
    __shared__ double lds_d[4];
    __shared__ double tile_rec[CT + 1];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t s = lower_bound(keyA, n, (uint64_t)c << 53), e = lower_bound(keyA, n, (uint64_t)(c + 1) << 53);
    if (t == 0) { cls_start[c] = s; if (c == (int)gridDim.x - 1) cls_start[c + 1] = e; }
    const int64_t nd = e - s;
    if (nd == 0) { if (t == 0) ap[c] = -1.0; return; }           // no detections of this class: rec = prec = ap = -1 (:334-336)
    const double np_ = (double)npos[c];
    const double eps = DBL_EPSILON;                              // np.finfo(np.float64).eps
    uint64_t carry = 0;                                          // tp << 32 | fp so far
    int64_t nchg = 0;                                            // change points of recall so far
    double prev = 0.0;                                           // mrec[0]
    for (int64_t base = s; base < e; base += CT) {
        const int64_t p = base + t;
        const uint8_t f = p < e ? flag[keyA[p] & ((1ull << KEY_IDX_BITS) - 1)] : 0;
        uint64_t v = (uint64_t)(f == 1) << 32 | (uint64_t)(f == 2);
        v = block_scan_incl(v, [](uint64_t x, uint64_t y) { return x + y; }, lds_u) + carry;
        const double tp = (double)(v >> 32), fp = (double)(v & 0xffffffffu);
        const double r = tp / np_;                               // tp / float(npos): NaN when npos == 0
        const double sum = tp + fp;
        const double pr = tp / (sum >= eps ? sum : eps);         // tp / np.maximum(tp + fp, eps)
        tile_rec[t + 1] = r;
        if (t == 0) tile_rec[0] = prev;
        __syncthreads();
        int chg = 0;
        if (p < e) {
            rec[p] = r;
            prec[p] = pr;
            chg = r != tile_rec[t];                              // mrec[i+1] != mrec[i] (NaN != anything)
        }
        const uint64_t cs = block_scan_incl((uint64_t)chg, [](uint64_t x, uint64_t y) { return x + y; }, lds_u);
        if (chg) pts[s + nchg + (int64_t)cs - 1] = (int32_t)(p - s);
        if (t == CT - 1) { lds_u[0] = v; lds_u[1] = cs; lds_d[0] = tile_rec[CT]; }
        __syncthreads();
        carry = lds_u[0]; nchg += (int64_t)lds_u[1]; prev = lds_d[0];
        __syncthreads();
    }
    double run = 0.0;                                            // mpre[n+1] sentinel; envelope = suffix max (prec is never NaN)
    const int64_t ntiles = (nd + CT - 1) / CT;
    for (int64_t tile = ntiles - 1; tile >= 0; --tile) {
        const int64_t p = s + tile * CT + (CT - 1 - t);          // thread t walks the tile backwards
        double v = p < e ? prec[p] : 0.0;
        v = block_scan_incl(v, [](double x, double y) { return x > y ? x : y; }, lds_d);
        v = v > run ? v : run;
        if (p < e) env[p] = v;
        if (t == CT - 1) lds_d[0] = v;
        __syncthreads();
        run = lds_d[0];
        __syncthreads();
    }
    __threadfence_block();
    if (use07) {
        if (t == 0) {
            double a = 0.0;
            for (int i = 0; i < 11; ++i) {                       // np.arange(0., 1.1, 0.1)[i] == i * 0.1
                const double th = (double)i * 0.1;
                int64_t lo = 0, hi = nd;                         // first j with rec[j] >= th (rec is non-decreasing; all NaN -> none)
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (rec[s + mid] >= th) hi = mid; else lo = mid + 1;
                }
                const double pv = lo < nd ? env[s + lo] : 0.0;   // np.max(prec[rec >= t]) or 0
                a = a + pv / 11.0;
            }
            ap[c] = a;
        }
        return;
    }
    // area: terms (mrec[i+1] - mrec[i]) * mpre[i+1] at the change points i in 0..nd-1, then i = nd (mrec 1, mpre 0) if it changes
    double* tm = terms + s + c;
    for (int64_t j = t; j < nchg; j += CT) {
        const int64_t i = pts[s + j];
        const double rprev = i == 0 ? 0.0 : rec[s + i - 1];
        tm[j] = (rec[s + i] - rprev) * env[s + i];
    }
    __syncthreads();
    if (t == 0) {
        int64_t m = nchg;
        const double rl = rec[e - 1];
        if (1.0 != rl) tm[m++] = (1.0 - rl) * 0.0;
        ap[c] = numpy_sum(tm, m);
    }
}

}  // namespace

// ---- state ----------------------------------------------------------------------------------------------------------------------
struct EvalState {
    int device = 0, C = 0;
    double ovthresh = 0.5;
    int64_t n = 0;                             // records ingested
    int n_img = 0;
    DevBuf<int32_t> soa;                       // [7][planes()]: img, cls, k, x1, y1, x2, y2 (tenths)
    int64_t planes() const { return (int64_t)(soa.cap() / 7); }
    DevBuf<int32_t> img_first;                 // [n_img]
    DevBuf<int32_t> geom_dev;
    PinnedBuf<int32_t> pinned;                 // offsets[B] read-back + geometry staging
    DevBuf<int> err_dev;
    std::vector<int32_t> gt;                   // [G][5] grouped by (image, class), file order inside
    std::vector<int32_t> gt_seg{0};            // [n_img * C + 1]
    std::vector<int64_t> npos;                 // [C] non-difficult GT
    // finish
    DevBuf<uint64_t> keyA, keyB;
    DevBuf<uint8_t> flag;
    DevBuf<double> rec, prec, env, terms, ap;
    DevBuf<int32_t> pts;
    DevBuf<int64_t> npos_dev, cls_start;
    DevBuf<int32_t> gt_dev, gt_seg_dev;
    bool finished = false;
    std::vector<int64_t> starts;               // [C+1] class segments of the last finish
};

int eval_create(int device, int C, double ovthresh, EvalState** out, std::string& err)
{
    if (C < 1 || C > 2000) { err = "yn_eval_create: num_classes must be 1..2000"; return 1; }
    if (!(ovthresh == ovthresh)) { err = "yn_eval_create: ovthresh is NaN"; return 1; }
    auto* e = new EvalState;
    e->device = device; e->C = C; e->ovthresh = ovthresh;
    e->npos.assign(C, 0);
    int r = e->err_dev.reserve(4);
    if (!r) r = e->pinned.reserve(64);
    if (!r) r = hipMemset(e->err_dev, 0, 16);
    if (r) { err = std::string("yn_eval_create: ") + hipGetErrorString((hipError_t)r); eval_destroy(e); return 1; }
    *out = e;
    return 0;
}

void eval_destroy(EvalState* e)
{
    if (!e) return;
    DeviceScope on(e->device);
    delete e;
}

int eval_reset(EvalState* e, hipStream_t s, std::string& err)
{
    EVCHK(hipStreamSynchronize(s));
    e->n = 0; e->n_img = 0;
    e->gt.clear(); e->gt_seg.assign(1, 0);
    e->npos.assign(e->C, 0);
    e->finished = false;
    EVCHK(hipMemsetAsync(e->err_dev, 0, 16, s));
    return 0;
}

// 0 ok, 1 error, 2 range mark (offsets[B] < 0): nothing added
int eval_add(EvalState* e, hipStream_t s, int B, const float* rec_dev, const int32_t* offsets_dev, const int32_t* geom,
             const int32_t* gt, const int32_t* gt_off, std::string& err)
{
    if (B <= 0 || !rec_dev || !offsets_dev || !geom || !gt_off) { err = "yn_eval_add: bad arguments"; return 1; }
    if (gt_off[0] != 0) { err = "yn_eval_add: gt_offsets[0] must be 0"; return 1; }
    for (int b = 0; b < B; ++b) {
        if (gt_off[b + 1] < gt_off[b]) { err = "yn_eval_add: gt_offsets must not decrease"; return 1; }
        const int32_t* g = geom + 7 * b;
        if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0 || g[6] <= 0) { err = "yn_eval_add: geometry needs positive w0, h0, rw, rh, side"; return 1; }
    }
    if (gt_off[B] > 0 && !gt) { err = "yn_eval_add: ground truth pointer is null"; return 1; }
    if ((int64_t)e->n_img + B >= (1 << 21)) { err = "yn_eval_add: more than 2^21 images"; return 1; }
    // the ground truth first (host only): validated before anything is changed
    const int C = e->C;
    std::vector<int> cnt(C);
    for (int b = 0; b < B; ++b) {
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int i = gt_off[b]; i < gt_off[b + 1]; ++i) {
            const int32_t* g = gt + 6 * (int64_t)i;
            if (g[4] < 0 || g[4] >= C) { err = "yn_eval_add: ground-truth class out of range"; return 1; }
            if (++cnt[g[4]] > EV_MAX_GT) { err = "yn_eval_add: more than 4096 ground-truth boxes of one class in one image"; return 1; }
        }
    }
    if (e->pinned.cap() < 1 + 7 * (size_t)B) {
        EVCHK(hipStreamSynchronize(s));
        EVCHK(e->pinned.reserve(1 + 7 * (size_t)B));
    }
    EVCHK(hipMemcpyAsync(e->pinned, offsets_dev + B, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));            // also retires the previous batch's use of the geometry staging
    const int32_t total = e->pinned[0];
    if (total < 0) { err = "yn_eval_add: offsets[B] is negative (split-f16 range mark): nothing added"; return 2; }
    if (e->n + total >= ((int64_t)1 << 31)) { err = "yn_eval_add: more than 2^31 - 1 records"; return 1; }
    // records: grow the SoA store (keeps what is there)
    if (e->n + total > e->planes()) {
        int64_t nc = e->planes() ? e->planes() : 4096;
        while (nc < e->n + total) nc *= 2;
        DevBuf<int32_t> p;                     // the seven planes move apart: copied by hand, swapped in when all of it has arrived
        EVCHK(p.reserve((size_t)nc * 7));
        if (e->n)
            for (int f = 0; f < 7; ++f)
                EVCHK(hipMemcpyAsync(p + f * nc, e->soa + f * e->planes(), (size_t)e->n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        EVCHK(hipStreamSynchronize(s));
        e->soa = std::move(p);
    }
    EVCHK(e->img_first.reserve_keep((size_t)e->n_img + B, (size_t)e->n_img, s, 1024));
    EVCHK(e->geom_dev.reserve(7 * (size_t)B, 1));
    memcpy(e->pinned + 1, geom, 7 * (size_t)B * sizeof(int32_t));
    EVCHK(hipMemcpyAsync(e->geom_dev, e->pinned + 1, 7 * (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int64_t threads = total > B ? total : B;
    hipLaunchKernelGGL(eval_ingest_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, rec_dev, offsets_dev, B,
                       (const int32_t*)e->geom_dev, C, e->n, e->n_img, e->soa, e->planes(), e->img_first, e->err_dev);
    EVCHK(hipGetLastError());
    // ground truth: per image, grouped by class in file order
    for (int b = 0; b < B; ++b) {
        for (int c = 0; c < C; ++c) {
            for (int i = gt_off[b]; i < gt_off[b + 1]; ++i) {
                const int32_t* g = gt + 6 * (int64_t)i;
                if (g[4] != c) continue;
                e->gt.insert(e->gt.end(), {g[0], g[1], g[2], g[3], g[5] ? 1 : 0});
                if (!g[5]) e->npos[c] += 1;
            }
            e->gt_seg.push_back((int32_t)(e->gt.size() / 5));
        }
    }
    e->n += total;
    e->n_img += B;
    e->finished = false;
    return 0;
}

static const char* err_text(int bits)
{
    if (bits & EV_ERR_SCORE) return "a detection score rounds outside 0.000..1.000";
    if (bits & EV_ERR_CLASS) return "a detection class is not an integer in 0..C-1";
    if (bits & EV_ERR_COORD) return "a detection coordinate in pixels is not finite or too large";
    return "an image holds 2^22 or more detections";
}

int eval_finish(EvalState* e, hipStream_t s, int use07, double* ap_host, int64_t* npos_host, int64_t* ndet_host, std::string& err)
{
    const int C = e->C;
    const int64_t n = e->n;
    int64_t npow = EV_LOCAL;
    while (npow < n) npow *= 2;
    const size_t m = (size_t)(n + C);
    EVCHK(e->keyA.reserve((size_t)npow));
    EVCHK(e->keyB.reserve((size_t)npow));
    EVCHK(e->flag.reserve(m));
    EVCHK(e->rec.reserve(m));
    EVCHK(e->prec.reserve(m));
    EVCHK(e->env.reserve(m));
    EVCHK(e->terms.reserve(m));
    EVCHK(e->pts.reserve(m));
    EVCHK(e->ap.reserve((size_t)C));
    EVCHK(e->npos_dev.reserve((size_t)C));
    EVCHK(e->cls_start.reserve((size_t)C + 1));
    EVCHK(e->gt_dev.reserve(e->gt.size() + 5, 1));
    EVCHK(e->gt_seg_dev.reserve(e->gt_seg.size(), 1));
    EVCHK(hipStreamSynchronize(s));
    if (!e->gt.empty()) EVCHK(hipMemcpyAsync(e->gt_dev, e->gt.data(), e->gt.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EVCHK(hipMemcpyAsync(e->gt_seg_dev, e->gt_seg.data(), e->gt_seg.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EVCHK(hipMemcpyAsync(e->npos_dev, e->npos.data(), C * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (n > 0) {
        hipLaunchKernelGGL(eval_keys_kernel, dim3((unsigned)((npow + 255) / 256)), dim3(256), 0, s, (const int32_t*)e->soa, e->planes(),
                           (const int32_t*)e->img_first, n, npow, e->keyA, e->keyB);
        bitonic_sort(e->keyA.get(), npow, s);
        bitonic_sort(e->keyB.get(), npow, s);
        const int64_t pairs = (int64_t)e->n_img * C;
        hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, (const uint64_t*)e->keyB, n,
                           (const int32_t*)e->soa, e->planes(), (const int32_t*)e->img_first, (const int32_t*)e->gt_dev,
                           (const int32_t*)e->gt_seg_dev, e->n_img, C, e->ovthresh, e->flag);
    }
    hipLaunchKernelGGL(eval_curve_kernel, dim3(C), dim3(CT), 0, s, (const uint64_t*)e->keyA, n, (const uint8_t*)e->flag,
                       (const int64_t*)e->npos_dev, use07, e->rec, e->prec, e->env, e->pts, e->terms, e->ap, e->cls_start);
    EVCHK(hipGetLastError());
    e->starts.assign(C + 1, 0);
    int bits = 0;
    EVCHK(hipMemcpyAsync(ap_host, e->ap, C * sizeof(double), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(e->starts.data(), e->cls_start, (C + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(&bits, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    if (bits) { err = std::string("yn_eval_finish: ") + err_text(bits); return 1; }
    for (int c = 0; c < C; ++c) {
        if (npos_host) npos_host[c] = e->npos[c];
        if (ndet_host) ndet_host[c] = e->starts[c + 1] - e->starts[c];
    }
    e->finished = true;
    return 0;
}

int eval_curve(EvalState* e, hipStream_t s, int cls, double* rec_host, double* prec_host, int64_t cap, std::string& err)
{
    if (!e->finished) { err = "yn_eval_curve: call yn_eval_finish first"; return 1; }
    if (cls < 0 || cls >= e->C) { err = "yn_eval_curve: class out of range"; return 1; }
    const int64_t s0 = e->starts[cls], nd = e->starts[cls + 1] - s0, m = nd < cap ? nd : cap;
    if (m > 0) {
        if (rec_host) EVCHK(hipMemcpyAsync(rec_host, e->rec + s0, m * sizeof(double), hipMemcpyDeviceToHost, s));
        if (prec_host) EVCHK(hipMemcpyAsync(prec_host, e->prec + s0, m * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    EVCHK(hipStreamSynchronize(s));
    return 0;
}

int eval_records(EvalState* e, hipStream_t s, int32_t* host, int64_t cap, std::string& err)
{
    const int64_t m = e->n < cap ? e->n : cap;
    int bits = 0;
    std::vector<int32_t> tmp((size_t)m * 7);
    for (int f = 0; f < 7 && m > 0; ++f)
        EVCHK(hipMemcpyAsync(tmp.data() + f * m, e->soa + f * e->planes(), m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(&bits, e->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    if (bits) { err = std::string("yn_eval_records: ") + err_text(bits); return 1; }
    for (int64_t i = 0; i < m; ++i)
        for (int f = 0; f < 7; ++f) host[i * 7 + f] = tmp[f * m + i];
    return 0;
}

void eval_size(const EvalState* e, int64_t* records, int64_t* images)
{
    if (records) *records = e->n;
    if (images) *images = e->n_img;
}

}  // namespace ynk
