// kernels_track.hip — detections tracked across video frames on the device: the step kernel, the output compaction and the state behind
// yn_track.  DESIGN.md §29 is the specification; tests/track_oracle.py restates it one float32 operation at a time and this file is built
// with -ffp-contract=off so that every product and sum below rounds where the oracle's does.
//
// One workgroup of 256 threads steps one frame of the call, that is one stream.  Thread r < max_tracks owns slot r and keeps its 27 state
// words in registers from the load to the store; the detections, the predicted boxes and the 128 x 128 IoU matrix (row stride 129 floats, so
// that a row scan by thread r and a column scan by thread c are both free of bank conflicts) live in LDS.  Selection, predict, the three
// matching stages, update, births and the frame's compacted output happen without a global round trip; a second, small launch sums the
// frames' counts and moves the rows to their place in the caller's buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "yn_devbuf.h"
#include "yn_eval_shared.h"
#include "yn_internal.h"

namespace ynk {

namespace {

constexpr int TRACK_MAX = 128;                  // slots per stream and detections per frame, at most
constexpr int TRACK_THREADS = 256;
constexpr int TRACK_LD = TRACK_MAX + 1;         // row stride of the IoU matrix
constexpr int TRACK_CHUNK = 256;                // frames per step launch: their stream indices travel in the kernel arguments
constexpr int TRACK_META = 5, TRACK_FILT = 22;
constexpr int T_FREE = 0, T_TENTATIVE = 1, T_CONFIRMED = 2, T_LOST = 3;
enum { CNT_STEPS, CNT_BIRTHS, CNT_DROPPED, CNT_OVERFLOW, CNT_IGNORED, CNT_MARKS, CNT_N };

struct TrackParams {
    float track_high, track_low, new_thresh, iou_high, iou_low, iou_new, w_pos, w_vel;
    int max_lost, min_hits, class_aware;
};

struct TrackStreams { uint16_t s[TRACK_CHUNK]; };

struct Coord { float p, v, P00, P01, P11; };    // one coordinate's constant-velocity filter

__device__ __forceinline__ void kf_initiate(Coord& c, float z, float s, const TrackParams& P)
{
    const float t0 = 2.0f * P.w_pos * s;
    const float t1 = 10.0f * P.w_vel * s;
    c.p = z; c.v = 0.0f; c.P00 = t0 * t0; c.P01 = 0.0f; c.P11 = t1 * t1;
}

__device__ __forceinline__ void kf_predict(Coord& c, float s, const TrackParams& P)
{
    const float q = P.w_pos * s;
    const float qv = P.w_vel * s;
    const float P00 = c.P00, P01 = c.P01, P11 = c.P11;
    c.p = c.p + c.v;
    c.P00 = ((P00 + 2.0f * P01) + P11) + q * q;
    c.P01 = P01 + P11;
    c.P11 = P11 + qv * qv;
}

__device__ __forceinline__ void kf_update(Coord& c, float z, float s, const TrackParams& P)
{
    const float q = P.w_pos * s;
    const float P00 = c.P00, P01 = c.P01, P11 = c.P11;
    const float S = P00 + q * q;
    const float K0 = P00 / S;
    const float K1 = P01 / S;
    const float r = z - c.p;
    c.p = c.p + K0 * r;
    c.v = c.v + K1 * r;
    c.P00 = P00 - (K0 * K0) * S;
    c.P01 = P01 - (K0 * K1) * S;
    c.P11 = P11 - (K1 * K1) * S;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN and the infinities

// rank of this thread among the threads of the block whose flag is set, and their number; ws is 4 ints of LDS
__device__ __forceinline__ int block_rank(bool f, int* ws, int& total)
{
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) ws[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < TRACK_THREADS / 64; ++i) {
        const int n = ws[i];
        if (i < w) off += n;
        total += n;
    }
    __syncthreads();
    return pre + off;
}

struct TrackLds {
    float iou[TRACK_MAX * TRACK_LD];
    float tx1[TRACK_MAX], ty1[TRACK_MAX], tx2[TRACK_MAX], ty2[TRACK_MAX], tcls[TRACK_MAX];
    float dx1[TRACK_MAX], dy1[TRACK_MAX], dx2[TRACK_MAX], dy2[TRACK_MAX], dscore[TRACK_MAX], dcls[TRACK_MAX];
    int tkind[TRACK_MAX];                       // the slot's state at the start of the step; 0 when it cannot be matched in this step
    int tmatch[TRACK_MAX], dmatch[TRACK_MAX], dhigh[TRACK_MAX];
    int rbest[TRACK_MAX], cbest[TRACK_MAX];
    int cand[TRACK_MAX];
    unsigned long long open[TRACK_THREADS / 64];
    int ws[TRACK_THREADS / 64];
};

// a wave-uniform 64-bit value in scalar registers, so that a loop over its bits is scalar control flow
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

// One greedy stage in rounds: every pair that is the best of its row (ties: lowest detection) and of its column (ties: lowest slot) among
// the open eligible pairs is taken, until a round takes none.  The same matching as taking the best open pair one at a time with ties to
// the lowest slot, then the lowest detection (tests/test_track_cpu.py).  Threads 0..127 are the rows, 128..255 the columns; the open rows
// and columns of a round are four ballots in LDS, and a scan walks the set bits of the other side's two words in ascending order, one LDS
// read per open candidate.  A thread scans again only when the best it holds has been taken.
__device__ __forceinline__ void match_stage(TrackLds& L, int max_tracks, int nd, float thr, unsigned kinds, int want_high)
{
    const int t = threadIdx.x;
    const bool is_row = t < TRACK_MAX;
    const int i = is_row ? t : t - TRACK_MAX;
    bool active = is_row ? (i < max_tracks && ((kinds >> L.tkind[i]) & 1u) && L.tmatch[i] < 0) : (i < nd && L.dhigh[i] == want_high && L.dmatch[i] < 0);
    int best = -1;
    bool stale = true;
    for (;;) {
        const unsigned long long mine = __ballot(active);
        if ((t & 63) == 0) L.open[t >> 6] = mine;               // words 0, 1: rows; 2, 3: columns
        __syncthreads();
        if (active && stale) {
            float bv = -1.0f;
            best = -1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                unsigned long long m = uniform64(L.open[(is_row ? 2 : 0) + h]);
                while (m) {
                    const int o = h * 64 + __builtin_ctzll(m);
                    m &= m - 1ull;
                    const float v = is_row ? L.iou[i * TRACK_LD + o] : L.iou[o * TRACK_LD + i];
                    if (v >= thr && v > bv) { bv = v; best = o; }
                }
            }
            if (best < 0) active = false;                       // the open set only shrinks: nothing will become eligible later
        }
        (is_row ? L.rbest : L.cbest)[i] = active ? best : -1;
        __syncthreads();
        int took = 0;
        if (is_row && active && L.cbest[best] == i) {
            L.tmatch[i] = best;
            L.dmatch[best] = i;
            active = false;
            took = 1;
        }
        if (!__syncthreads_or(took)) break;
        if (active) {
            if (is_row) stale = L.dmatch[best] >= 0;
            else { stale = L.tmatch[best] >= 0; if (L.dmatch[i] >= 0) active = false; }
        }
    }
}

__global__ __launch_bounds__(TRACK_THREADS) void track_step_kernel(TrackStreams table, int b0, int B, int max_tracks, int max_dets, TrackParams P,
                                                                   const float* __restrict__ rec, const int32_t* __restrict__ offsets, long long rec_capacity,
                                                                   int32_t* __restrict__ meta_g, float* __restrict__ filt_g, int32_t* __restrict__ next_id_g,
                                                                   float* __restrict__ stage_rec, int32_t* __restrict__ stage_ids,
                                                                   int32_t* __restrict__ stage_count, unsigned long long* __restrict__ counters)
{
    __shared__ TrackLds L;
    const int t = threadIdx.x;
    const int b = b0 + (int)blockIdx.x;
    if (offsets[B] < 0) {                                       // the split-f16 range mark: no state word changes
        if (b == 0 && t == 0) atomicAdd(&counters[CNT_MARKS], 1ull);
        if (t == 0) stage_count[b] = 0;
        return;
    }
    const int stream = table.s[blockIdx.x];
    const bool owner = t < max_tracks;
    int32_t* meta = meta_g + ((size_t)stream * max_tracks + (owner ? t : 0)) * TRACK_META;
    float* filt = filt_g + ((size_t)stream * max_tracks + (owner ? t : 0)) * TRACK_FILT;

    // ---- the slot's state, in registers ----
    int state = T_FREE, id = 0, hits = 0, lost_age = 0, mdet = -1;
    float cls = 0.0f, score = 0.0f;
    Coord k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = Coord{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (owner) {
        state = meta[0]; id = meta[1]; hits = meta[2]; lost_age = meta[3]; mdet = meta[4];
        cls = filt[0]; score = filt[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = Coord{filt[2 + 5 * j], filt[3 + 5 * j], filt[4 + 5 * j], filt[5 + 5 * j], filt[6 + 5 * j]};
    }
    const int next_id = next_id_g[stream];

    // ---- 1. detections: the usable records in record order, the first max_dets of them ----
    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > rec_capacity ? rec_capacity : lo);
    hi = hi < lo ? lo : (hi > rec_capacity ? rec_capacity : hi);
    int n_usable = 0;
    for (long long base = lo; base < hi; base += TRACK_THREADS) {
        const long long i = base + t;
        float x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f, sc = 0.0f, cl = 0.0f;
        bool usable = false;
        if (i < hi) {
            const float* r = rec + i * 6;
            x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3]; sc = r[4]; cl = r[5];
            usable = finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2) && x2 > x1 && y2 > y1 && sc >= P.track_low;
        }
        int total;
        const int at = n_usable + block_rank(usable, L.ws, total);
        if (usable && at < max_dets) {
            L.dx1[at] = x1; L.dy1[at] = y1; L.dx2[at] = x2; L.dy2[at] = y2; L.dscore[at] = sc; L.dcls[at] = cl;
            L.dhigh[at] = sc >= P.track_high ? 1 : 0;
            L.dmatch[at] = -1;
        }
        n_usable += total;
    }
    const int nd = n_usable < max_dets ? n_usable : max_dets;

    // ---- 2. predict ----
    const int state0 = state;
    if (owner) {
        bool valid = false;
        if (state0 != T_FREE) {
            if (state0 == T_LOST) { k[2].v = 0.0f; k[3].v = 0.0f; }
            const float sw = k[2].p, sh = k[3].p;
            kf_predict(k[0], sw, P); kf_predict(k[1], sh, P); kf_predict(k[2], sw, P); kf_predict(k[3], sh, P);
            const float w = k[2].p, h = k[3].p;
            valid = finite_f(w) && finite_f(h) && w > 0.0f && h > 0.0f;
            L.tx1[t] = k[0].p - 0.5f * w; L.ty1[t] = k[1].p - 0.5f * h; L.tx2[t] = k[0].p + 0.5f * w; L.ty2[t] = k[1].p + 0.5f * h;
            L.tcls[t] = cls;
        }
        L.tkind[t] = valid ? state0 : 0;
        L.tmatch[t] = -1;
    }
    __syncthreads();

    // ---- 3. IoU: thread t fills column t & 127 of the rows of its half ----
    {
        const int c = t & (TRACK_MAX - 1);
        if (c < nd) {
            const float bx1 = L.dx1[c], by1 = L.dy1[c], bx2 = L.dx2[c], by2 = L.dy2[c], bcls = L.dcls[c];
            const float area_b = (bx2 - bx1) * (by2 - by1);
            for (int r = t >> 7; r < max_tracks; r += 2) {
                float v = -1.0f;
                if (L.tkind[r] != 0 && (!P.class_aware || L.tcls[r] == bcls)) {
                    const float ax1 = L.tx1[r], ay1 = L.ty1[r], ax2 = L.tx2[r], ay2 = L.ty2[r];
                    float iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1);
                    float ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
                    iw = iw > 0.0f ? iw : 0.0f;
                    ih = ih > 0.0f ? ih : 0.0f;
                    const float inter = iw * ih;
                    const float area_a = (ax2 - ax1) * (ay2 - ay1);
                    const float uni = (area_a + area_b) - inter;
                    v = uni > 0.0f ? inter / uni : 0.0f;
                }
                L.iou[r * TRACK_LD + c] = v;
            }
        }
    }
    __syncthreads();

    // ---- 4. matching ----
    match_stage(L, max_tracks, nd, P.iou_high, 1u << T_CONFIRMED | 1u << T_LOST, 1);
    match_stage(L, max_tracks, nd, P.iou_low, 1u << T_CONFIRMED, 0);
    match_stage(L, max_tracks, nd, P.iou_new, 1u << T_TENTATIVE, 1);

    // ---- 5. / 6. matched and unmatched tracks ----
    if (owner && state0 != T_FREE) {
        const int c = L.tmatch[t];
        mdet = c;
        if (c >= 0) {
            const float x1 = L.dx1[c], y1 = L.dy1[c], x2 = L.dx2[c], y2 = L.dy2[c];
            const float sw = k[2].p, sh = k[3].p;
            kf_update(k[0], 0.5f * (x1 + x2), sw, P); kf_update(k[1], 0.5f * (y1 + y2), sh, P);
            kf_update(k[2], x2 - x1, sw, P); kf_update(k[3], y2 - y1, sh, P);
            score = L.dscore[c]; cls = L.dcls[c];
            hits += 1; lost_age = 0;
            if (state0 == T_LOST || (state0 == T_TENTATIVE && hits >= P.min_hits)) state = T_CONFIRMED;
        } else if (state0 == T_CONFIRMED) {
            state = T_LOST; lost_age = 1;
        } else {
            if (state0 == T_LOST) lost_age += 1;
            if (state0 == T_TENTATIVE || lost_age > P.max_lost) state = T_FREE;
        }
        if (state == T_FREE) {
            id = 0; hits = 0; lost_age = 0; cls = 0.0f; score = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = Coord{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        }
    }

    // ---- 7. births: the n-th candidate in detection order takes the n-th free slot ----
    int n_cand, n_free;
    const bool is_cand = t < nd && L.dhigh[t] == 1 && L.dmatch[t] < 0 && L.dscore[t] >= P.new_thresh;
    const int crank = block_rank(is_cand, L.ws, n_cand);
    if (is_cand) L.cand[crank] = t;
    const bool is_free = owner && state == T_FREE;
    const int frank = block_rank(is_free, L.ws, n_free);        // its barriers publish L.cand
    const int n_born = n_cand < n_free ? n_cand : n_free;
    if (is_free && frank < n_born) {
        const int c = L.cand[frank];
        const float x1 = L.dx1[c], y1 = L.dy1[c], x2 = L.dx2[c], y2 = L.dy2[c];
        const float w = x2 - x1, h = y2 - y1;
        kf_initiate(k[0], 0.5f * (x1 + x2), w, P); kf_initiate(k[1], 0.5f * (y1 + y2), h, P); kf_initiate(k[2], w, w, P); kf_initiate(k[3], h, h, P);
        cls = L.dcls[c]; score = L.dscore[c];
        state = P.min_hits <= 1 ? T_CONFIRMED : T_TENTATIVE;
        id = next_id + frank; hits = 1; lost_age = 0; mdet = c;
    }

    // ---- 8. output: confirmed tracks matched or born in this step, in slot order, into the frame's rows of the staging buffers ----
    int n_out;
    const bool emit = owner && state == T_CONFIRMED && mdet >= 0;
    const int orank = block_rank(emit, L.ws, n_out);
    if (emit) {
        float* o = stage_rec + ((size_t)b * max_tracks + orank) * 6;
        o[0] = k[0].p - 0.5f * k[2].p; o[1] = k[1].p - 0.5f * k[3].p; o[2] = k[0].p + 0.5f * k[2].p; o[3] = k[1].p + 0.5f * k[3].p;
        o[4] = score; o[5] = cls;
        stage_ids[(size_t)b * max_tracks + orank] = id;
    }

    // ---- the state goes back ----
    if (owner) {
        meta[0] = state; meta[1] = id; meta[2] = hits; meta[3] = lost_age; meta[4] = mdet;
        filt[0] = cls; filt[1] = score;
#pragma unroll
        for (int j = 0; j < 4; ++j) { filt[2 + 5 * j] = k[j].p; filt[3 + 5 * j] = k[j].v; filt[4 + 5 * j] = k[j].P00; filt[5 + 5 * j] = k[j].P01; filt[6 + 5 * j] = k[j].P11; }
    }
    if (t == 0) {
        next_id_g[stream] = next_id + n_born;
        stage_count[b] = n_out;
        atomicAdd(&counters[CNT_STEPS], 1ull);
        if (n_born) atomicAdd(&counters[CNT_BIRTHS], (unsigned long long)n_born);
        if (n_cand > n_born) atomicAdd(&counters[CNT_DROPPED], (unsigned long long)(n_cand - n_born));
        if (n_usable > nd) atomicAdd(&counters[CNT_OVERFLOW], (unsigned long long)(n_usable - nd));
        if (hi - lo > n_usable) atomicAdd(&counters[CNT_IGNORED], (unsigned long long)(hi - lo - n_usable));
    }
}

// frame b's rows move from the staging buffers to out_offsets[b] = the sum of the counts before it; the last block writes out_offsets[B]
__global__ __launch_bounds__(TRACK_THREADS) void track_finish_kernel(int B, int max_tracks, const int32_t* __restrict__ offsets,
                                                                     const float* __restrict__ stage_rec, const int32_t* __restrict__ stage_ids,
                                                                     const int32_t* __restrict__ stage_count, float* __restrict__ out_rec,
                                                                     int32_t* __restrict__ out_ids, int32_t* __restrict__ out_offsets)
{
    __shared__ int ws[TRACK_THREADS / 64];
    const int t = threadIdx.x, b = blockIdx.x;
    if (offsets[B] < 0) {
        if (t == 0) { out_offsets[b] = 0; if (b == B - 1) out_offsets[B] = -1; }
        return;
    }
    int part = 0;
    for (int i = t; i < b; i += TRACK_THREADS) part += stage_count[i];
    for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
    if ((t & 63) == 0) ws[t >> 6] = part;
    __syncthreads();
    const int start = ws[0] + ws[1] + ws[2] + ws[3];
    const int n = stage_count[b];
    if (t == 0) { out_offsets[b] = start; if (b == B - 1) out_offsets[B] = start + n; }
    for (int i = t; i < n * 6; i += TRACK_THREADS) out_rec[(size_t)start * 6 + i] = stage_rec[(size_t)b * max_tracks * 6 + i];
    for (int i = t; i < n; i += TRACK_THREADS) out_ids[(size_t)start + i] = stage_ids[(size_t)b * max_tracks + i];
}

// stream < 0: every stream and the counters
__global__ void track_reset_kernel(int stream, int streams, int max_tracks, int32_t* __restrict__ meta, float* __restrict__ filt,
                                   int32_t* __restrict__ next_id, unsigned long long* __restrict__ counters)
{
    const int s0 = stream < 0 ? 0 : stream, n = (stream < 0 ? streams : 1) * max_tracks;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        int32_t* m = meta + ((size_t)s0 * max_tracks + i) * TRACK_META;
        float* f = filt + ((size_t)s0 * max_tracks + i) * TRACK_FILT;
        m[0] = 0; m[1] = 0; m[2] = 0; m[3] = 0; m[4] = -1;
        for (int j = 0; j < TRACK_FILT; ++j) f[j] = 0.0f;
    }
    if (i < (stream < 0 ? streams : 1)) next_id[s0 + i] = 1;
    if (stream < 0 && i < CNT_N) counters[i] = 0ull;
}

}  // namespace

struct TrackState {
    int device = 0, streams = 0, max_tracks = 0, max_dets = 0;
    TrackParams P{};
    DevBuf<int32_t> meta;                                       // [streams][max_tracks][5]
    DevBuf<float> filt;                                         // [streams][max_tracks][22]
    DevBuf<int32_t> next_id;                                    // [streams]
    DevBuf<float> stage_rec;                                    // [streams][max_tracks][6]: a call's frame b writes its rows at b
    DevBuf<int32_t> stage_ids, stage_count;
    DevBuf<unsigned long long> counters;
    std::vector<unsigned char> seen;                            // the duplicate check of update()
};

int track_device(const TrackState* t) { return t->device; }

void track_destroy(TrackState* t)
{
    if (!t) return;
    DeviceScope on(t->device);
    delete t;
}

static void reset_launch(TrackState* t, hipStream_t s, int stream)
{
    const int n = (stream < 0 ? t->streams : 1) * t->max_tracks;
    hipLaunchKernelGGL(track_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, s, stream, t->streams, t->max_tracks, t->meta, t->filt, t->next_id, t->counters);
}

int track_create(int device, hipStream_t s, int streams, int max_tracks, int max_dets, const float* pf, const int32_t* pi, TrackState** out, std::string& err)
{
    if (streams < 1 || streams > 4096) { err = "yn_track_create: streams " + std::to_string(streams) + " outside 1..4096"; return 1; }
    if (max_tracks < 1 || max_tracks > TRACK_MAX) { err = "yn_track_create: max_tracks " + std::to_string(max_tracks) + " outside 1..128"; return 1; }
    if (max_dets < 1 || max_dets > TRACK_MAX) { err = "yn_track_create: max_dets " + std::to_string(max_dets) + " outside 1..128"; return 1; }
    TrackParams P{0.5f, 0.1f, 0.6f, 0.2f, 0.5f, 0.3f, 1.0f / 20.0f, 1.0f / 160.0f, 30, 2, 1};
    if (pf) P = TrackParams{pf[0], pf[1], pf[2], pf[3], pf[4], pf[5], pf[6], pf[7], pi[0], pi[1], pi[2]};
    static const char* const names[8] = {"track_high", "track_low", "new_thresh", "iou_high", "iou_low", "iou_new", "w_pos", "w_vel"};
    const float v[8] = {P.track_high, P.track_low, P.new_thresh, P.iou_high, P.iou_low, P.iou_new, P.w_pos, P.w_vel};
    for (int i = 0; i < 8; ++i)
        if (!(std::fabs(v[i]) <= 3.402823466e38f)) { err = std::string("yn_track_create: ") + names[i] + " is not finite"; return 1; }
    if (P.track_low > P.track_high) { err = "yn_track_create: track_low is above track_high"; return 1; }
    for (int i = 3; i < 6; ++i)
        if (!(v[i] > 0.0f && v[i] <= 1.0f)) { err = std::string("yn_track_create: ") + names[i] + " outside (0, 1]"; return 1; }
    if (P.max_lost < 0) { err = "yn_track_create: max_lost is negative"; return 1; }
    if (P.min_hits < 1) { err = "yn_track_create: min_hits is below 1"; return 1; }
    P.class_aware = P.class_aware ? 1 : 0;
    auto* t = new TrackState;
    t->device = device; t->streams = streams; t->max_tracks = max_tracks; t->max_dets = max_dets; t->P = P;
    t->seen.assign(streams, 0);
    const size_t slots = (size_t)streams * max_tracks;
    int r = t->meta.reserve(slots * TRACK_META);
    if (!r) r = t->filt.reserve(slots * TRACK_FILT);
    if (!r) r = t->next_id.reserve((size_t)streams);
    if (!r) r = t->stage_rec.reserve(slots * 6);
    if (!r) r = t->stage_ids.reserve(slots);
    if (!r) r = t->stage_count.reserve((size_t)streams);
    if (!r) r = t->counters.reserve(CNT_N);
    if (!r) { reset_launch(t, s, -1); r = hipGetLastError(); }
    if (!r) r = hipStreamSynchronize(s);
    if (r) { err = std::string("yn_track_create: ") + hipGetErrorString((hipError_t)r); track_destroy(t); return 1; }
    *out = t;
    return 0;
}

int track_reset(TrackState* t, hipStream_t s, int stream, std::string& err)
{
    if (stream < -1 || stream >= t->streams) { err = "yn_track_reset: stream " + std::to_string(stream) + " outside -1.." + std::to_string(t->streams - 1); return 1; }
    reset_launch(t, s, stream);
    EVCHK(hipGetLastError());
    return 0;
}

int track_update(TrackState* t, hipStream_t s, int B, const int32_t* stream_host, const float* rec_dev, const int32_t* offsets_dev, int64_t rec_capacity,
                 float* out_rec, int32_t* out_ids, int32_t* out_offsets, std::string& err)
{
    if (B < 0) { err = "yn_track_update: negative batch"; return 1; }
    if (B > t->streams) { err = "yn_track_update: " + std::to_string(B) + " frames for " + std::to_string(t->streams) + " streams"; return 1; }
    if (rec_capacity < 0 || rec_capacity > ((int64_t)1 << 31) - 1) { err = "yn_track_update: rec_capacity outside 0..2^31 - 1"; return 1; }
    if (B == 0) {                                               // an empty call is not an error: no stream is stepped
        if (out_offsets) EVCHK(hipMemsetAsync(out_offsets, 0, sizeof(int32_t), s));
        return 0;
    }
    if ((!rec_dev && rec_capacity > 0) || !offsets_dev || !out_rec || !out_ids || !out_offsets) { err = "yn_track_update: null pointer"; return 1; }
    std::fill(t->seen.begin(), t->seen.end(), 0);
    for (int b = 0; b < B; ++b) {
        const int st = stream_host ? stream_host[b] : b;
        if (st < 0 || st >= t->streams) {
            err = "yn_track_update: frame " + std::to_string(b) + " names stream " + std::to_string(st) + ", outside 0.." + std::to_string(t->streams - 1);
            return 1;
        }
        if (t->seen[st]) { err = "yn_track_update: stream " + std::to_string(st) + " is named twice"; return 1; }
        t->seen[st] = 1;
    }
    for (int b0 = 0; b0 < B; b0 += TRACK_CHUNK) {
        TrackStreams table{};
        const int m = std::min(TRACK_CHUNK, B - b0);
        for (int i = 0; i < m; ++i) table.s[i] = (uint16_t)(stream_host ? stream_host[b0 + i] : b0 + i);
        hipLaunchKernelGGL(track_step_kernel, dim3(m), dim3(TRACK_THREADS), 0, s, table, b0, B, t->max_tracks, t->max_dets, t->P, rec_dev, offsets_dev,
                           (long long)rec_capacity, t->meta, t->filt, t->next_id, t->stage_rec, t->stage_ids, t->stage_count, t->counters);
    }
    hipLaunchKernelGGL(track_finish_kernel, dim3(B), dim3(TRACK_THREADS), 0, s, B, t->max_tracks, offsets_dev, t->stage_rec, t->stage_ids, t->stage_count,
                       out_rec, out_ids, out_offsets);
    EVCHK(hipGetLastError());
    return 0;
}

int track_state(TrackState* t, hipStream_t s, int stream, int32_t* meta_host, float* filt_host, int32_t* next_id, std::string& err)
{
    if (stream < 0 || stream >= t->streams) { err = "yn_track_state: stream " + std::to_string(stream) + " outside 0.." + std::to_string(t->streams - 1); return 1; }
    const size_t at = (size_t)stream * t->max_tracks;
    if (meta_host) EVCHK(hipMemcpyAsync(meta_host, t->meta + at * TRACK_META, (size_t)t->max_tracks * TRACK_META * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (filt_host) EVCHK(hipMemcpyAsync(filt_host, t->filt + at * TRACK_FILT, (size_t)t->max_tracks * TRACK_FILT * sizeof(float), hipMemcpyDeviceToHost, s));
    if (next_id) EVCHK(hipMemcpyAsync(next_id, t->next_id + stream, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    return 0;
}

int track_status(TrackState* t, hipStream_t s, int64_t* counters6, std::string& err)
{
    unsigned long long c[CNT_N] = {};
    EVCHK(hipMemcpyAsync(c, t->counters, sizeof(c), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    for (int i = 0; i < CNT_N; ++i) counters6[i] = (int64_t)c[i];
    return 0;
}

}  // namespace ynk
