// kernels_chain.hip — multi-layer tile kernel: unit_chain_kernel (one launch per stride-1 ShuffleV2 unit, cut at the depthwise conv).
#include "yn_internal.h"
#include "yn_device.h"

#include <cstdlib>
#include <type_traits>

namespace ynk {

// -------------------------------------------------------------------------------------------------
// Stride-1 ShuffleV2 units as a chain of ONE kernel per unit (backbone/shufflenetv2.py:53-63, 70-72, 14-28).
//
//   unit i:   x = [x1 | x2],  t = relu(pw1_i(x2)),  y = relu(pw2_i(dw_i(t))),  out = shuffle(cat(x1, y))
//
// Cutting the chain at the unit INPUT needs pw1 on a halo (shuffle_unit_kernel: slower than three kernels).  Cutting it at the
// depthwise conv does not: everything after dw_i is pixel-local, including the next unit's pw1, because the shuffle makes
// x2_{i+1} = interleave(x1[bf/2:], y[bf/2:]) of the SAME pixel.  So the kernel of unit i is
//   1. dw_i on the block's BM pixels, read from global (t_i, neighbours through L1/L2; XCD-contiguous tiles keep them in one
//      L2), each output computed once -> LDS tile T [BM][bf+2];
//   2. GEMM y = relu(T * W2 + b2) (f32 MFMA, A fragments from T, W2 streamed through one LDS buffer with register prefetch);
//   3. y -> T (in place, after a barrier);  interleave pass: out[:, 0:bf] = interleave(x1[0:bf/2], y[0:bf/2]) -> global (the
//      next unit's pass-through half — the only part of `out` a later kernel reads), x2' = interleave(x1[bf/2:], y[bf/2:])
//      -> registers -> T;  (last unit of a stage: the whole `out` row goes to global and the kernel ends here)
//   4. GEMM t_{i+1} = relu(T * W1' + b1') -> global.
// Per unit: 1 launch instead of 3, 4 tensors of [M][bf] through memory instead of 8, no halo recompute.  All sums run in the
// order of the separate kernels (same fma chain in the depthwise conv, same k order in the GEMMs): bit-identical results.
// Measured (tools/phase_timing.sh chain2, stage 3, M = 21 632, bf = 116; cycles per block): depthwise phase 20 k, GEMM 13.1 k each (two
// co-resident blocks share the MFMA pipe: 2 x 7.4 k of MFMA issue), y->T 5.5 k, interleave 3.2 k, epilogue 5.6 k = 39 us per unit
// against 46 us for the three kernels (stage 2: 42 vs 66, stage 4: 47 vs 45).  All blocks of the launch are resident at once and run their phases in lockstep, so the depthwise phase is the
// whole chip fetching its ~35 MB at the same time (bandwidth-bound, MFMAs idle) and the GEMM phases leave the memory system
// idle; overlapping them needs a persistent block that requests tile i+1's window (direct-to-LDS loads) while tile i is in
// its GEMMs — the next step for this kernel.  (Tried: the GEMM weights register-direct from L2 instead of through LDS, which
// removes the chunk barriers — GEMM phase 13.7 k -> 22 k cycles: the 8-byte per-lane weight loads are slower than the barriers;
// and starting the second block of a CU 8 k / 16 k / 24 k cycles late (s_sleep on odd HW wave slots) so that co-resident blocks
// are out of phase: 40.5 / 42.7 / 44.8 us against 42 us, i.e. nothing — with 338 blocks only a third of the CUs hold two.)
// -------------------------------------------------------------------------------------------------
template <int WM, int WN, int NT, int V>
__global__ __launch_bounds__(256, 2) void unit_chain_kernel(ChainArgs a)
{
    typedef typename VecT<V>::type vec;
    constexpr int BM = 32 * WM, BN = 32 * NT * WN, KP = 16, BS = BN * 2, B_PER = KP * BN / 512, G = V / 2;
    constexpr int MAXB = (BM * (BN / (2 * G)) + 255) / 256;     // interleave items per thread and half (upper bound: bf <= BN)
    static_assert(WM * WN == 4 && B_PER >= 1, "4 waves");
    extern __shared__ __attribute__((aligned(16))) float uc_smem[];
    const int bf = a.bf, CS = bf + 2, W = a.W, H = a.H, HW = H * W;
    float* T = uc_smem;                                      // [BM][CS]
    float* Bs = uc_smem + ((BM * CS + 3) & ~3);              // [2][KP][BS]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int m0 = (int)xcd_block(blockIdx.x, gridDim.x) * BM;
    if (m0 >= a.M) return;
    const int nchunks = (bf + 2 * KP - 1) / (2 * KP), kp_total = bf >> 1;

    // GEMM weights: chunks of KP k-pairs through TWO LDS buffers, requested TWO chunks ahead into two register sets, so a
    // chunk's loads have two chunk-times (~4 k cycles) to arrive and there is one barrier per chunk.
    float4 regA[B_PER], regB[B_PER];
    auto prefetch_b = [&](float4 (&reg)[B_PER], const float* Wp, int c) {
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int idx = t + 256 * i;
            const int kp = idx / (BN / 2), c4 = idx - kp * (BN / 2);
            const int kpg = c * KP + kp;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (kpg < kp_total) v = *reinterpret_cast<const float4*>(Wp + ((size_t)kpg * a.Npad + c4 * 2) * 2);
            reg[i] = v;
        }
    };
    auto stage_b = [&](float4 (&reg)[B_PER], int buf) {
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int idx = t + 256 * i;
            const int kp = idx / (BN / 2), c4 = idx - kp * (BN / 2);
            *reinterpret_cast<float4*>(Bs + buf * KP * BS + kp * BS + c4 * 4) = reg[i];
        }
    };
#ifdef YN_EXP_TIMING
    long long TS[8]; int tsn = 0;
#define YN_TS() TS[tsn++] = __builtin_readcyclecounter()
#else
#define YN_TS()
#endif
    YN_TS();
    // the two GEMM biases of this lane's columns: requested now, used tens of microseconds later (a dependent load at the start
    // of an epilogue is a full memory latency with nothing to hide it)
    float bias2[NT], bias1n[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = wn * NT * 32 + nt * 32 + l31;
        bias2[nt] = n < bf ? a.b2[n] : 0.0f;
        bias1n[nt] = (a.Wp1n && n < bf) ? a.b1n[n] : 0.0f;
    }

    // The pass-through half x1 is only needed by the interleave pass after the first GEMM: request it now, so that its
    // latency hides behind the depthwise conv and the GEMM.  Item it = (row, G consecutive j of the first half-row); the same
    // item also owns the j + bf/2 of the second half-row (xg / xl).
    const int hipr = bf / (2 * G), jhi = bf >> 1;          // items per half row; first j of the second half (bf/2 is a multiple of G)
    float2 xg[MAXB], xl[MAXB];                               // G == 1 uses .x only
    auto x1_prefetch = [&]() {
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int it = t + 256 * i;
        const int r = it / hipr, j0 = (it - r * hipr) * G;
        const int m = m0 + r < a.M ? m0 + r : a.M - 1;
        xg[i] = make_float2(0.0f, 0.0f); xl[i] = xg[i];
        if (it < BM * hipr) {
            const float* px = a.x1 + (size_t)m * a.x1_ld + a.x1_off + j0;
            if constexpr (G == 2) {
                xg[i] = *reinterpret_cast<const float2*>(px);
                xl[i] = *reinterpret_cast<const float2*>(px + jhi);
            } else {
                xg[i].x = px[0];
                xl[i].x = px[jhi];
            }
        }
    }
    };

    // ---- 1. depthwise 3x3 of the block's pixels -> T ---------------------------------------------------------
    {
        const int cgn = bf / V, ppl = 256 / cgn;
        const int cg = t % cgn, pl = t / cgn, c = cg * V;
        const bool worker = pl < ppl;                        // 256 is not a multiple of the channel groups: a few threads idle
        {
            // Thread = (channel group, runs of R consecutive flat pixels).  Neighbour (dy, dx) of flat pixel p is flat pixel
            // p + dy*W + dx wherever it exists, so the 3 x (R+2) window of a run is three runs of consecutive pixels: 18 loads
            // (one batch, no masks: addresses clamped into the tensor) feed R = 4 outputs; image borders are handled when the
            // window is used (select 0 per output and tap).
            constexpr int R = 4;
            auto issue = [&](int run, vec (&win)[3][R + 2]) {
                const int q0 = m0 + run * R - 1;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int i = 0; i < R + 2; ++i) {
                        int q = q0 + (dy - 1) * W + i;
                        q = q < 0 ? 0 : (q >= a.M ? a.M - 1 : q);
                        win[dy][i] = *reinterpret_cast<const vec*>(a.t1 + (size_t)q * a.t1_ld + a.t1_off + c);
                    }
            };
            // the nine taps and the bias of this thread's channel group live in registers (the kernel runs at two waves per SIMD
            // either way; from LDS they cost 72 ds_read_b128 per thread)
            vec w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const vec*>(a.wdw + k * bf + c);
            const vec bias = *reinterpret_cast<const vec*>(a.bdw + c);
            auto finish = [&](int run, vec (&win)[3][R + 2]) {
                const int mrun = m0 + run * R;
                const int rem0 = (mrun < a.M ? mrun : m0) % HW;  // one division per run; the R pixels advance by one column
                int y = rem0 / W, x = rem0 - y * W;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int r = run * R + i;
                    const bool live = mrun + i < a.M;
                    const bool yk[3] = {live && y >= 1, live, live && y + 1 < H};
                    const bool xk[3] = {x >= 1, true, x + 1 < W};
                    vec acc = bias;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const bool ok = yk[ky] && xk[kx];
                            vec v = win[ky][i + kx];
                            if constexpr (V == 4) v = make_float4(ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
                            else v = make_float2(ok ? v.x : 0.0f, ok ? v.y : 0.0f);
                            vfma(acc, v, w[ky * 3 + kx]);
                        }
                    acc = vact(acc, a.dw_act);
                    float* d = T + r * CS + c;                   // row stride CS*4 bytes is only 8-byte aligned
                    if constexpr (V == 4) {
                        *reinterpret_cast<float2*>(d) = make_float2(acc.x, acc.y);
                        *reinterpret_cast<float2*>(d + 2) = make_float2(acc.z, acc.w);
                    } else {
                        *reinterpret_cast<float2*>(d) = acc;
                    }
                    if (++x == W) { x = 0; if (++y == H) y = 0; }
                }
            };
            // One window in flight per thread: the latency is hidden by the other blocks of the CU (a second window in flight
            // costs 72 registers and an occupancy step: measured 2x slower).
            vec win[3][R + 2];
            // request order = completion order (vmcnt is in-order): the first window, then the GEMM's first weight chunk, then x1
            if (worker) issue(pl, win);
            prefetch_b(regA, a.Wp2, 0);
            x1_prefetch();
            stage_b(regA, 0);                                // GEMM entry state: chunk 0 in buffer 0, chunk 1 requested into regA
            if (nchunks > 1) prefetch_b(regA, a.Wp2, 1);
            if (worker) {
                for (int run = pl; run < BM / R; run += ppl) {
                    finish(run, win);
                    if (run + ppl < BM / R) issue(run + ppl, win);
                }
            }
        }
        for (int r = t; r < BM; r += 256) *reinterpret_cast<float2*>(T + r * CS + bf) = make_float2(0.0f, 0.0f);   // pad columns (K tail)
    }
    __syncthreads();
    YN_TS();

    // ---- GEMM: acc = T[BM][bf] * Wp (chunk 0 already staged in Bs) --------------------------------------------
    f32x16 acc[NT];
    auto mfma_chunk = [&](int c, int buf) {
        const int krem = bf - c * 2 * KP;
        const int nq = krem >= 2 * KP ? KP / 2 : ((krem + 3) >> 2);
        const float* Ab = T + (wm * 32 + l31) * CS + c * 2 * KP + 2 * h;
        const float* Bb = Bs + buf * KP * BS + (wn * NT * 32 + l31) * 2 + h * BS;
        float2 av = *reinterpret_cast<const float2*>(Ab);
        float2 bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float2*>(Bb + nt * 64);
#pragma unroll
        for (int q = 0; q < KP / 2; ++q) {
            if (q < nq) {                                   // wave-uniform
                float2 av_n = av, bv_n[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bv_n[nt] = bv[nt];
                if (q + 1 < nq) {
                    av_n = *reinterpret_cast<const float2*>(Ab + 4 * (q + 1));
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv_n[nt] = *reinterpret_cast<const float2*>(Bb + 2 * (q + 1) * BS + nt * 64);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[nt].x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[nt].y, acc[nt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                av = av_n;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bv[nt] = bv_n[nt];
            }
        }
    };
    // entry state: chunk 0 staged in buffer 0 (visible), chunk 1 requested into regA
    auto gemm = [&](const float* Wp) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][k] = 0.0f;
        for (int c = 0; c < nchunks; c += 2) {
            if (c + 2 < nchunks) prefetch_b(regB, Wp, c + 2);
            mfma_chunk(c, 0);
            if (c + 1 >= nchunks) break;
            stage_b(regA, 1);                               // buffer 1 was last read two chunks ago, before the previous barrier
            __syncthreads();
            if (c + 3 < nchunks) prefetch_b(regA, Wp, c + 3);
            mfma_chunk(c + 1, 1);
            if (c + 2 < nchunks) {
                stage_b(regB, 0);
                __syncthreads();
            }
        }
    };
    gemm(a.Wp2);
    YN_TS();
    if (a.Wp1n) prefetch_b(regA, a.Wp1n, 0);
    __syncthreads();                                        // all waves are done reading T and Bs

    // ---- 3. y = act(acc + b2) -> T (in place) -----------------------------------------------------------------
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = wn * NT * 32 + nt * 32 + l31;
        if (n < bf) {
            const float bias = bias2[nt];
#pragma unroll
            for (int r = 0; r < 16; ++r) T[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * CS + n] = apply_act(acc[nt][r] + bias, a.act2);
        }
    }
    if (a.Wp1n) {
        stage_b(regA, 0);
        if (nchunks > 1) prefetch_b(regA, a.Wp1n, 1);
    }
    __syncthreads();
    YN_TS();

    // interleave pass.  Item = (row, G consecutive j): (x1[j], y[j], ...) -> 2G consecutive output channels 2j..
    // First half-row (j < bf/2) -> global; second half-row -> global too (last unit: whole `out` row) or -> x2' in T.
    float2 yl[MAXB];
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {
        const int it = t + 256 * i;
        const int r = it / hipr, j0 = (it - r * hipr) * G, m = m0 + r;
        yl[i] = make_float2(0.0f, 0.0f);
        if (it < BM * hipr) {
            float2 y = make_float2(0.0f, 0.0f);
            if constexpr (G == 2) { y = *reinterpret_cast<const float2*>(T + r * CS + j0); yl[i] = *reinterpret_cast<const float2*>(T + r * CS + jhi + j0); }
            else { y.x = T[r * CS + j0]; yl[i].x = T[r * CS + jhi + j0]; }
            if (m < a.M) {
                float* o = a.out + (size_t)m * a.out_ld + 2 * j0;
                if constexpr (G == 2) {
                    *reinterpret_cast<float4*>(o) = make_float4(xg[i].x, y.x, xg[i].y, y.y);
                    if (!a.Wp1n) *reinterpret_cast<float4*>(o + 2 * jhi) = make_float4(xl[i].x, yl[i].x, xl[i].y, yl[i].y);
                } else {
                    *reinterpret_cast<float2*>(o) = make_float2(xg[i].x, y.x);
                    if (!a.Wp1n) *reinterpret_cast<float2*>(o + 2 * jhi) = make_float2(xl[i].x, yl[i].x);
                }
            }
        }
    }
    if (!a.Wp1n) return;
    __syncthreads();                                        // every read of y is done: T may be overwritten
#pragma unroll
    for (int i = 0; i < MAXB; ++i) {                        // ... and x2' = interleave(x1[bf/2:], y[bf/2:]) into T
        const int it = t + 256 * i;
        const int r = it / hipr, c0 = 2 * (it - r * hipr) * G;
        if (it < BM * hipr) {
            *reinterpret_cast<float2*>(T + r * CS + c0) = make_float2(xl[i].x, yl[i].x);
            if constexpr (G == 2) *reinterpret_cast<float2*>(T + r * CS + c0 + 2) = make_float2(xl[i].y, yl[i].y);
        }
    }
    __syncthreads();

    YN_TS();
    // ---- 4. the next unit's pw1 on x2' -> global ------------------------------------------------------------------
    gemm(a.Wp1n);
    YN_TS();
    GemmArgs e{};
    e.out = a.t1n; e.out_ld = bf; e.out_off = 0; e.M = a.M; e.N = bf; e.Npad = a.Npad; e.bias = a.b1n; e.act = a.act1n; e.pass = nullptr;
    gemm_epilogue<NT>(e, acc, m0 + wm * 32, wn * NT * 32, (bf & 3) == 0, lane, bias1n);
#ifdef YN_EXP_TIMING
    YN_TS();
    if (t == 0 && (blockIdx.x % 97) == 5)
        printf("chain bf %d blk %d start %lld dw %lld gemm1 %lld y %lld interleave %lld gemm2 %lld epi %lld\n", bf, (int)blockIdx.x, TS[0], TS[1] - TS[0], TS[2] - TS[1], TS[3] - TS[2], TS[4] - TS[3], TS[5] - TS[4], TS[6] - TS[5]);
#endif
#undef YN_TS
}

// -------------------------------------------------------------------------------------------------
// The same chain on the split-f16 family (gemm_split_kernel's numerics: x = hi + lo*2^-11, three f16 MFMAs per product, K in order
// => bit-identical to the three-kernel path on gemm_split_kernel).  With the GEMM phases 4-5x shorter the unit is the depthwise
// (memory) phase plus two short matrix phases, so ONE launch per unit beats three again.  LDS: the depthwise output / x2' as two
// planes of halves P[2][BM][PS] (A operands); the weights go through registers.
// -------------------------------------------------------------------------------------------------

// -------------------------------------------------------------------------------------------------
// unit_chain2_kernel (round 3).  What changed against the round-2 form, and why (tools/phase_timing.sh chain2: of a block's ~50 k
// cycles only the first ~14 k move data from HBM; the rest is a chain of latency-bound phases with the memory idle):
//   * the fp32 tile T32 [BM][bf+2] for y and its two passes are gone.  The accumulator layout already gives every lane ONE column n
//     and 16 rows: the lane loads x1[row][n] itself (16 * NT scalar loads at kernel start, 128-byte rows per half-wavefront), and after the
//     first GEMM turns each accumulator value straight into its final place - out[row][2n .. 2n+1] = (x1, y) as one 8-byte
//     store (columns n < bf/2 - or all of them in the last unit of a stage), or x2'[2(n - bf/2) ..] = split(x1, y) into the
//     operand planes (columns n >= bf/2).  One barrier and ~9 k cycles of LDS round trips less per block; LDS 78 -> 64 KB at bf = 116.
//   * (measured and dropped: a BALANCED launch - 96-row tiles on six wavefronts, ceil(M / CUs) = 88 live pixels each, one workgroup
//     per CU instead of 64-pixel tiles that leave 82 CUs with two: the kernel went 25.7 -> 25.2 us, because six wavefronts sharing the
//     LDS and matrix pipes stretch both GEMM phases from 6 k to 8.2 k cycles, and the 81 KB workgroup cost 6 % of the four-stream
//     throughput, 39.2 k -> 36.8 k images/s)
//   * K goes through LDS in chunks of KC = 64 instead of 32: half the barrier pairs inside the two GEMMs (two chunks at bf = 116;
//     a chunk round costs ~2 k cycles whatever it multiplies).  Same k order (16-deep steps in sequence, zero-padded tail skipped):
//     bit-identical to the round-2 form and to gemm_split_kernel.
// -------------------------------------------------------------------------------------------------
#ifndef YN_UC2_OCC_NARROW
#define YN_UC2_OCC_NARROW 3                                 // workgroups per CU the 58-channel (stage 2) instantiation is compiled for
#endif
template <int WM, int WN, int NT, int V, int D>             // D: 16-deep k-steps of weight fragments in flight per wavefront
__global__ __launch_bounds__(64 * WM * WN, (WM * WN != 4 ? 1 : ((NT == 1 && V == 2) ? YN_UC2_OCC_NARROW : 2))) void unit_chain2_kernel(ChainArgs a)
{
    typedef typename VecT<V>::type vec;
    constexpr int BM = 32 * WM, BN = 32 * NT * WN, NTHR = 64 * WM * WN;
    extern __shared__ __attribute__((aligned(16))) float uc2_smem[];
    const int bf = a.bf, W = a.W, H = a.H, HW = H * W;
    const int KQ = (bf + 7) >> 3, PS = plane_stride(bf), S = (KQ + 1) >> 1;     // S: 16-deep k-steps of a GEMM
    h16* Ph = reinterpret_cast<h16*>(uc2_smem);                     // [BM][PS]
    h16* Pl = Ph + BM * PS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int m0 = (int)xcd_block(blockIdx.x, gridDim.x) * BM;
    if (m0 >= a.M) return;
    const int nrows = a.M - m0 < BM ? a.M - m0 : BM;                    // live rows of this tile

#ifdef YN_EXP_TIMING
    long long TS[8]; int tsn = 0;
#define YN_TS() TS[tsn++] = __builtin_readcyclecounter()
#else
#define YN_TS()
#endif
    YN_TS();
    // Round 4: the GEMM weights never pass through LDS (down2_kernel's finding): a lane's B fragment of a k-step is 16 contiguous bytes
    // of the pre-split pack, so every wavefront streams the fragments of ITS columns straight from L2 into registers, D k-steps ahead - no
    // chunk barriers, no staging pass, half the LDS (the first form walked K in chunks of 64 through LDS: two barrier rounds of ~2 k
    // cycles per GEMM whatever they multiplied, and a 2.3 k staging pass between the GEMMs).  Same k order (16-deep steps in sequence):
    // the same bits.
    h16x8 bq[D][NT][2];
    auto load_b = [&](const void* Wh_, const void* Wl_, int s, h16x8 (&dst)[NT][2]) {
        const h16* Wh = reinterpret_cast<const h16*>(Wh_);
        const h16* Wl = reinterpret_cast<const h16*>(Wl_);
        // NO masks (round 5): a masked load is USED where it is issued - eight v_and per fragment - and hipcc then waits for it there: every k-step
        // of the walk drained the vector-memory counter (vmcnt(3) ... vmcnt(0) in front of its MFMAs) and cost a full L2 round trip, D deep or
        // not.  Clamped addresses instead: an octet past K (kq = KQ, odd octet counts) meets the planes' zero K tail, a column past Npad is
        // never stored, a step past the walk reads its A fragment from the zero tail (a_col below).  Finite weights x 0: exact zeros, as before.
        const int kq = min(s * 2 + h, KQ - 1);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = min(wn * NT * 32 + nt * 32 + l31, a.Npad - 1);
            const size_t off = ((size_t)kq * a.Npad + n) * 8;
            dst[nt][0] = *reinterpret_cast<const h16x8*>(Wh + off);
            dst[nt][1] = *reinterpret_cast<const h16x8*>(Wl + off);
        }
    };
    auto prime_b = [&](const void* Wh, const void* Wl) {
#pragma unroll
        for (int j = 0; j < D; ++j) load_b(Wh, Wl, j, bq[j]);
    };
    float amax = 0.0f;                                                   // range guard (yn_split.h)
    auto split_store = [&](int r, int c, float v0, float v1) {           // two adjacent channels of row r -> both planes
        h16x2 hi, lo;
        amax = range_track(range_track(amax, v0), v1);
        hi[0] = (h16)v0; hi[1] = (h16)v1;
        lo[0] = split_lo(v0, hi[0]); lo[1] = split_lo(v1, hi[1]);
        *reinterpret_cast<h16x2*>(Ph + r * PS + c) = hi;
        *reinterpret_cast<h16x2*>(Pl + r * PS + c) = lo;
    };

    float bias2[NT], bias1n[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = wn * NT * 32 + nt * 32 + l31;
        bias2[nt] = n < bf ? a.b2[n] : 0.0f;
        bias1n[nt] = (a.Wp1n && n < bf) ? a.b1n[n] : 0.0f;
    }
    const int jhi = bf >> 1;
    // the pass-through half in the ACCUMULATOR layout: x1v[nt][r] = x1[row(r)][n(nt)] (needed after the first GEMM)
    float x1v[NT][16];
    // wave-uniform base pointers + 32-bit lane offsets: the loads / stores below then use the saddr form instead of a 64-bit
    // multiply-add per access
    const char* x1_base = reinterpret_cast<const char*>(a.x1 + (size_t)m0 * a.x1_ld + a.x1_off);
    auto x1_prefetch = [&]() {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = wn * NT * 32 + nt * 32 + l31;
            const bool nok = n < bf;
            const unsigned mk = opaque_mask(nok);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int rr = row < nrows ? row : nrows - 1;           // clamped into the tile (idle rows are never stored)
                const unsigned off = (unsigned)(rr * a.x1_ld + (nok ? n : 0)) * 4u;
                x1v[nt][r] = __uint_as_float(__float_as_uint(*reinterpret_cast<const float*>(x1_base + off)) & mk);
            }
        }
    };

    // ---- 1. depthwise 3x3 of the block's pixels -> split planes (the same fma chain as dwconv3x3_kernel) ------------------------
    {
        const int cgn = bf / V, ppl = NTHR / cgn;
        const int cg = t % cgn, pl = t / cgn, c = cg * V;
        const bool worker = pl < ppl;
        constexpr int R = 4;
        auto issue = [&](int run, vec (&win)[3][R + 2]) {
            const int q0 = m0 + run * R - 1;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int i = 0; i < R + 2; ++i) {
                    int q = q0 + (dy - 1) * W + i;
                    q = q < 0 ? 0 : (q >= a.M ? a.M - 1 : q);
                    win[dy][i] = *reinterpret_cast<const vec*>(a.t1 + (size_t)q * a.t1_ld + a.t1_off + c);
                }
        };
        vec w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const vec*>(a.wdw + k * bf + c);
        const vec bias = *reinterpret_cast<const vec*>(a.bdw + c);
        auto finish = [&](int run, vec (&win)[3][R + 2]) {
            const int mrun = m0 + run * R;
            const int rem0 = (mrun < a.M ? mrun : m0) % HW;
            int y = rem0 / W, x = rem0 - y * W;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int r = run * R + i;
                const bool live = r < nrows;
                const bool yk[3] = {live && y >= 1, live, live && y + 1 < H};
                const bool xk[3] = {x >= 1, true, x + 1 < W};
                vec acc = bias;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const bool ok = yk[ky] && xk[kx];
                        vec v = win[ky][i + kx];
                        if constexpr (V == 4) v = make_float4(ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
                        else v = make_float2(ok ? v.x : 0.0f, ok ? v.y : 0.0f);
                        vfma(acc, v, w[ky * 3 + kx]);
                    }
                acc = vact(acc, a.dw_act);
                if constexpr (V == 4) { split_store(r, c, acc.x, acc.y); split_store(r, c + 2, acc.z, acc.w); }
                else split_store(r, c, acc.x, acc.y);
                if (++x == W) { x = 0; if (++y == H) y = 0; }
            }
        };
        const int nruns = (nrows + R - 1) / R;
        prime_b(a.Ws2h, a.Ws2l);                            // (requested before the windows: they return first)
        // (both windows of a thread in flight at once - the registers are there since the weights stopped passing through LDS - measured
        //  the same: 24.5 vs 25.1 us per stage-3 unit, 40.8 vs 41.2 k images/s; one window keeps the kernel at 203 registers)
        vec win[3][R + 2];
        if (worker && pl < nruns) issue(pl, win);
        if (worker) {
            for (int run = pl; run < nruns; run += ppl) {
                finish(run, win);
                if (run + ppl < nruns) issue(run + ppl, win);
            }
        }
        // requested only now: the window registers are free again, and these loads (x1 is a quarter of the unit's traffic) fly during
        // the first GEMM, when the memory system would otherwise sit idle
        x1_prefetch();
        // K tail: the columns [bf, PS) of both planes are zero (they meet zero weight rows, but must not be NaN bit patterns)
        const int padn = PS - bf;
        for (int i = t; i < BM * padn; i += NTHR) { const int r = i / padn, c2 = bf + i - r * padn; Ph[r * PS + c2] = (h16)0.0f; Pl[r * PS + c2] = (h16)0.0f; }
    }
    __syncthreads();
    YN_TS();

    f32x16 acc0[NT], acc1[NT];
    // entry state: the fragments of steps 0 .. D-1 of this matrix are in flight (prime_b).  Steps past the last one (at most D - 1 of them)
    // multiply the zero K tail of the A rows by whatever fragment the clamped load brought: exact zeros, no branch around the loads
    auto gemm = [&](const void* Wh, const void* Wl) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) { acc0[i][k] = 0.0f; acc1[i][k] = 0.0f; }
        for (int s0 = 0; s0 < S; s0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int s = s0 + j;
                const int a_col = s < S ? s * 16 + h * 8 : PS - 8;      // past the walk: the last 16 bytes of the row's zero K tail (plane_stride)
                const h16x8 ah = *reinterpret_cast<const h16x8*>(Ph + (wm * 32 + l31) * PS + a_col);
                const h16x8 al = *reinterpret_cast<const h16x8*>(Pl + (wm * 32 + l31) * PS + a_col);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    split_mfma(ah, al, bq[j][nt][0], bq[j][nt][1], acc0[nt], acc1[nt]);
                }
                load_b(Wh, Wl, s + D, bq[j]);                   // (clamped beyond the last step)
                __builtin_amdgcn_sched_barrier(0);              // HERE, behind the MFMAs that freed the slot: hipcc sank all D steps' loads to the end of
            }                                                   // the unrolled group, where the next group needs them at once (a round trip per group)
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) split_join(acc0[nt], acc1[nt]);
    };
    gemm(a.Ws2h, a.Ws2l);
    YN_TS();
    if (a.Wp1n) prime_b(a.Ws1h, a.Ws1l);                               // the next GEMM's first fragments fly during the epilogue
    __syncthreads();                                                    // all waves are done reading the planes
#ifdef YN_EXP_TIMING
    const long long t_bar = __builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t_x1 = __builtin_readcyclecounter();
#endif

    // ---- 2. y = act(acc + b2) straight to its final place: (x1, y) pairs -> global, or split into the planes as x2' ---------------
    const bool last = a.Wp1n == nullptr;
    const bool uniform8 = (nrows & 7) == 0;                             // wave-uniform: a row group of 8 is live or idle as a whole
    char* out_base = reinterpret_cast<char*>(a.out + (size_t)m0 * a.out_ld);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = wn * NT * 32 + nt * 32 + l31;
        const float bias = bias2[nt];
        const bool to_global = n < (last ? bf : jhi);
        const bool to_plane = !last && n >= jhi && n < bf;
        float y[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = apply_act(acc0[nt][r] + bias, a.act2);
        // ONE exec region per destination, scalar branches per row group (a per-value `if` compiles to a branch + waits around every
        // store: measured 200 cycles each)
        if (uniform8) {
#pragma unroll
            for (int g8 = 0; g8 < 4; ++g8) {
                if (wm * 32 + 8 * g8 < nrows) {                         // scalar condition
                    if (to_global) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int row = wm * 32 + q + 8 * g8 + 4 * h;
                            *reinterpret_cast<float2*>(out_base + (unsigned)(row * a.out_ld + 2 * n) * 4u) = make_float2(x1v[nt][4 * g8 + q], y[4 * g8 + q]);
                        }
                    }
                    if (to_plane) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) split_store(wm * 32 + q + 8 * g8 + 4 * h, 2 * (n - jhi), x1v[nt][4 * g8 + q], y[4 * g8 + q]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < nrows) {
                    if (to_global) *reinterpret_cast<float2*>(out_base + (unsigned)(row * a.out_ld + 2 * n) * 4u) = make_float2(x1v[nt][r], y[r]);
                    if (to_plane) split_store(row, 2 * (n - jhi), x1v[nt][r], y[r]);
                }
            }
        }
    }
    YN_TS();
    if (last) { range_report(a.ovf, amax); return; }
    __syncthreads();

    // ---- 3. the next unit's pw1 on x2' -> global -------------------------------------------------------------------------------
    YN_TS();
    gemm(a.Ws1h, a.Ws1l);
    YN_TS();
    GemmArgs e{};
    e.out = a.t1n; e.out_ld = bf; e.out_off = 0; e.M = m0 + nrows; e.N = bf; e.Npad = a.Npad; e.bias = a.b1n; e.act = a.act1n; e.pass = nullptr;      // rows beyond the tile's live ones are not stored
    gemm_epilogue<NT>(e, acc0, m0 + wm * 32, wn * NT * 32, (bf & 3) == 0, lane, bias1n);
    range_report(a.ovf, amax);
#ifdef YN_EXP_TIMING
    YN_TS();
    if (t == 0 && (blockIdx.x % 97) == 5)
        printf("chain2 bf %d blk %d dw %lld gemm1 %lld fused-epi %lld (barrier %lld x1wait %lld work %lld) stage %lld gemm2 %lld epi %lld total %lld\n", bf, (int)blockIdx.x, TS[1] - TS[0], TS[2] - TS[1],
               TS[3] - TS[2], t_bar - TS[2], t_x1 - t_bar, TS[3] - t_x1, TS[4] - TS[3], TS[5] - TS[4], TS[6] - TS[5], TS[6] - TS[0]);
#endif
#undef YN_TS
}

static size_t unit_chain2_lds(int bf, int BM)
{
    const int PS = plane_stride(bf);
    return (size_t)2 * BM * PS * 2;                          // the two operand planes; the weights go through registers
}

static size_t unit_chain_lds(int bf, int BM, int BN) { return ((size_t)((BM * (bf + 2) + 3) & ~3) + (size_t)2 * 16 * BN * 2) * sizeof(float); }

// false when no instantiated tile covers the shape (Npad must be one block column; bf % 4 == 0 or the 2-channel variant)
// s == nullptr && dry: only answer whether an instantiated tile covers the shape (run_unit_chain asks before it launches anything)
static bool unit_chain_dispatch(const ChainArgs& a, hipStream_t s, bool dry)
{
    if ((a.bf & 1) || a.Npad < a.bf) return false;
    const bool v4 = (a.bf & 3) == 0 && ((a.t1_ld | a.t1_off | a.x1_ld | a.x1_off | a.out_ld) & 3) == 0;
    if (!v4 && (((a.t1_ld | a.t1_off | a.out_ld) & 1) != 0 || 256 / (a.bf / 2) < 1)) return false;
    if (v4 && 256 / (a.bf / 4) < 1) return false;
#define YN_UC(WMv, WNv, NTv, Vv)                                                                                       \
    {                                                                                                                  \
        constexpr int BM = 32 * WMv, BN = 32 * NTv * WNv;                                                              \
        const size_t lds = unit_chain_lds(a.bf, BM, BN);                                                               \
        if (lds > 160 * 1024) return false;                                                                            \
        if (dry) return true;                                                                                          \
        static unsigned long long attr = 0;                                                                                      \
        if (attr_pending(attr)) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(unit_chain_kernel<WMv, WNv, NTv, Vv>),    \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); } \
        set_last_kernel_name("unit_chain_kernel<" #WMv "," #WNv "," #NTv "," #Vv ">");                                      \
        hipLaunchKernelGGL((unit_chain_kernel<WMv, WNv, NTv, Vv>), dim3(xcd_grid((a.M + BM - 1) / BM)), dim3(256), lds, s, a); \
        return true;                                                                                                   \
    }
#define YN_UC2(WMv, WNv, NTv, Vv, KCv)                                                                                 \
    {                                                                                                                  \
        constexpr int BM = 32 * WMv, BN = 32 * NTv * WNv;                                                              \
        const size_t lds = unit_chain2_lds(a.bf, BM);                                                                  \
        if (lds > 160 * 1024) return false;                                                                            \
        if (dry) return true;                                                                                          \
        static unsigned long long attr = 0;                                                                            \
        if (attr_pending(attr)) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(unit_chain2_kernel<WMv, WNv, NTv, Vv, KCv>), \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }              \
        set_last_kernel_name("unit_chain2_kernel<" #WMv "," #WNv "," #NTv "," #Vv "," #KCv ">");                        \
        hipLaunchKernelGGL((unit_chain2_kernel<WMv, WNv, NTv, Vv, KCv>), dim3(xcd_grid((a.M + BM - 1) / BM)), dim3(64 * WMv * WNv), lds, s, a); \
        return true;                                                                                                   \
    }
    if (a.Ws2h) {
        // round 5: the persistent, software-pipelined form where it applies (kernels_pipe.hip); coverage is still decided by the tiles below
        if (!dry && launch_unit_pipe(a, s)) return true;
        if (a.Npad == 64 && !v4) YN_UC2(2, 2, 1, 2, 4)
        if (a.Npad == 64 && v4) YN_UC2(2, 2, 1, 4, 4)
        // small maps (one image): 32-row tiles - twice the workgroups, and a workgroup's serial chain (one depthwise round instead of two,
        // half the epilogue rows) is what a launch of a few dozen workgroups costs
        constexpr int small_m = 4096;
        if (a.Npad == 128 && v4 && a.M <= small_m) YN_UC2(1, 4, 1, 4, 4)
        if (a.Npad == 128 && v4) YN_UC2(2, 2, 2, 4, 3)
        if (a.Npad == 256 && v4) YN_UC2(1, 4, 2, 4, 3)          // 32-row tiles, four wavefronts x 64 columns (NT = 4 would need 128 accumulator + 64 pass-through registers)
        if (a.Npad == 32 && v4) YN_UC2(4, 1, 1, 4, 4)
        if (a.Npad == 96 && v4) YN_UC2(4, 1, 3, 4, 2)
        return false;
    }
#undef YN_UC2
    const int tiles64 = (a.M + 63) / 64;
    if (a.Npad == 64 && !v4) YN_UC(2, 2, 1, 2)
    if (a.Npad == 64 && v4) YN_UC(2, 2, 1, 4)
    if (a.Npad == 128 && v4) YN_UC(2, 2, 2, 4)                 // (a 32-row tile, <1,4,1,4>, measured the same: 42.4 vs 41.4 us)
    if (a.Npad == 256 && v4) { if (tiles64 >= 256) YN_UC(2, 2, 4, 4) else YN_UC(1, 4, 2, 4) }
    if (a.Npad == 32 && v4) YN_UC(4, 1, 1, 4)
    if (a.Npad == 96 && v4) YN_UC(4, 1, 3, 4)
#undef YN_UC
    return false;
}
// -------------------------------------------------------------------------------------------------
// A STRIDE-2 ShuffleV2 unit (backbone/shufflenetv2.py:30-51, 73-74) as one kernel:
//     branch 2:  y1 = relu(pw1(x)) at H x W  ->  y2 = dw3x3_s2(y1) at H/2 x W/2  ->  y3 = relu(pw2(y2))
//     branch 1:  z1 = dw3x3_s2(x)  ->  z2 = relu(pw(z1))                                  out = shuffle(cat(z2, y3))
// y1 is the largest tensor of the network (stage 2: 104 x 104 x 58 per image, 80 MB per 32-image step written and read back once) and the
// launches around it cost their full duration even with four streams (profiles/r06_ablation_4stream.txt: the big-tensor regions do not overlap with
// anything).  One tile = 8 x 4 OUTPUT pixels of one image: pw1 on the 17 x 9 input pixels the tile's depthwise windows cover (20 %
// recomputed on tile borders; K = cin <= 32 is one chunk), y1 in an fp32 LDS tile (zero outside the image: the depthwise conv pads its
// INPUT), depthwise -> split planes, pw2 (K = bf <= 64: two chunks) on wavefronts 0..NP-1 while wavefronts NP..2NP-1 run branch 1's
// pointwise conv, the concat + shuffle happens in an LDS tile and all four wavefronts store it in 16-byte row pieces.  x is read once (x 1.2) and `out` written once: 80 MB per step instead of
// 360 MB in five launches.  Every sum runs in the order of gemm_split_kernel / dwconv3x3_kernel: bit-identical to the five launches
// (test_down_unit_is_bit_identical).
// The kernel is a software pipeline (round 4).  With one tile per workgroup the load phase was 10 k of a workgroup's 25 k cycles (one
// memory round trip, 34 eight-byte loads per thread with a cache line per lane) at two workgroups of four wavefronts per CU - nothing to
// hide it behind.  So:
//   * a workgroup WALKS tiles (XCD-contiguous: workgroup i of XCD x takes tiles x*TL + i, + G/8, ...) and requests the next tile's input
//     window right after the barrier that frees the registers of the current one: the round trip runs under phases 2-5;
//   * the window is loaded as what it is - nine contiguous runs of 17 pixels x cin floats - with 16-byte loads (4-5 per thread, eight
//     cache lines per wavefront instruction instead of 64), split into the A planes AND kept as fp32 in LDS: branch 1's depthwise conv
//     reads its stride-2 windows there;
//   * every weight is loop-invariant: the B fragments of a wavefront's columns (16 contiguous bytes of the pre-split pack per lane and
//     k-step - down2_kernel's register-direct form) are loaded ONCE per workgroup into 48 registers, like the depthwise taps.  No
//     weight ever passes through LDS.  LDS 78 KB with the fp32 window: two workgroups per CU.
// -------------------------------------------------------------------------------------------------
// The widths are template parameters (the model family has two shapes here: (cin, bf) = (24, 58) at 1.0x and (24, 24) at 0.5x; anything else
// takes the down2 path, down_unit_covers): every item loop has a compile-time trip count and is unrolled - the LDS reads of a wavefront's
// GEMM-1 items and of a thread's depthwise outputs are issued together, the depthwise fma chains interleave - and the per-tile index
// arithmetic divides by constants: 48.9 -> 37.4 us at 416 x 416, bs = 32.
template <int CIN, int BF, bool RELU>                        // RELU: the three pointwise convs end in ReLU, the depthwise convs in nothing (ShuffleNetV2)
__global__ __launch_bounds__(256, 2) void down_unit_pipe_kernel(DownArgs a, int tiles)
{
    constexpr int NP = (BF + 31) / 32;
    constexpr int TW = 8, TH = 4, WW = 2 * TW + 1, WH = 2 * TH + 1, NPIX = WW * WH, RT1 = (NPIX + 31) / 32;
    constexpr int BN = 32 * NP, AST1 = 32 + 8, AST2 = BN + 8, NO = TW * TH, KS2 = 2 * NP;
    constexpr int bf = BF, CS = bf + 2, cin = CIN, cq = cin >> 2;
    constexpr int NLD = (WH * WW * cq + 255) / 256;                  // 16-byte window pieces per thread
    static_assert(CIN >= 16 && CIN <= 32 && !(CIN & 3) && BF <= 64 && !(BF & 1) && BF / 2 <= 256, "down_unit_covers");
    extern __shared__ __attribute__((aligned(16))) float du_smem[];
    h16* A1h = reinterpret_cast<h16*>(du_smem);                  // [RT1*32][AST1] x 2: pw1's operand planes
    h16* A1l = A1h + RT1 * 32 * AST1;
    h16* A2h = A1h;                                                // behind GEMM 1: [NO][AST2] x 2 (pw2), then [NO][AST1] x 2 (branch 1)
    h16* A2l = A2h + NO * AST2;
    h16* A3h = A2l + NO * AST2;
    h16* A3l = A3h + NO * AST1;
    float* X32 = du_smem + RT1 * 32 * AST1;                          // [RT1*32][cin]: the window in fp32 (zero outside the image)
    float* T32 = X32 + RT1 * 32 * cin;                               // [RT1*32][CS]: y1 (zero outside the image), later branch 1's tile
    unsigned char* inside = reinterpret_cast<unsigned char*>(T32 + RT1 * 32 * CS);      // [RT1*32]

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), l31 = lane & 31, h = lane >> 5;
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    const int tx_n = (Wo + TW - 1) / TW, ty_n = (Ho + TH - 1) / TH, per_img = tx_n * ty_n;
    constexpr int KQ1 = (cin + 7) >> 3, KQ2 = (bf + 7) >> 3;
    // the walk: XCD x = blockIdx & 7 owns tiles [x * TL, (x + 1) * TL)
    const int TL = (tiles + 7) >> 3, GL = (int)(gridDim.x >> 3);
    const int tbase = (int)(blockIdx.x & 7u) * TL;
    int tl = (int)(blockIdx.x >> 3);
    if (tl >= TL || tbase + tl >= tiles) return;
    auto act_pw = [&](float v, int act) { return RELU ? __builtin_fmaxf(v, 0.0f) : apply_act(v, act); };

#ifdef YN_EXP_TIMING
    long long TS[8]; int tsn = 0;
#define YN_TS() if (tsn < 8) TS[tsn++] = __builtin_readcyclecounter()
#else
#define YN_TS()
#endif
    YN_TS();
    // ---- loop invariants: depthwise taps and biases of both branches, the B fragments of this wavefront's columns --------------------
    constexpr int cp_n = bf >> 1, ppl = 256 / cp_n, NI2 = (NO + ppl - 1) / ppl;      // channel pairs, pixel lanes, outputs per thread of branch 2's depthwise conv
    const int cp = t % cp_n, dpl = t / cp_n, dc = cp * 2;
    const bool dworker = dpl < ppl;
    float2 wd[9], bd = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = dworker ? *reinterpret_cast<const float2*>(a.wdw + k * bf + dc) : make_float2(0.0f, 0.0f);
    if (dworker) bd = *reinterpret_cast<const float2*>(a.bdw + dc);
    constexpr int c1_n = cin >> 1, p1_n = 256 / c1_n;
    const int c1 = (t % c1_n) * 2, p1 = t / c1_n;
    constexpr int NI1 = (NO + p1_n - 1) / p1_n;                      // 32 output pixels over >= 16 pixel lanes (cin <= 32): at most two
    float2 w1d[9], b1d;
#pragma unroll
    for (int k = 0; k < 9; ++k) w1d[k] = *reinterpret_cast<const float2*>(a.wdw1 + k * cin + c1);
    b1d = *reinterpret_cast<const float2*>(a.bdw1 + c1);
    // GEMM 1: items it = (row tile, column tile) = 3 - wave, 7 - wave, ... - the wavefronts that run pw2 and the stores take the smaller share
    const int it0 = 3 - wave;
    const int nt1 = (NP == 2) ? (it0 & 1) : 0;                       // the stride 4 is even: a wavefront's column tile never changes
    const bool pw2_wave = wave < NP, b1_wave = wave >= NP && wave < 2 * NP;
    const int nt2 = pw2_wave ? wave : wave - NP;
    auto frag = [&](const void* Wh_, const void* Wl_, int ks, int KQ, int n, bool use, h16x8& bh, h16x8& bl) {
        const int kq = ks * 2 + h;
        const bool ok = use && kq < KQ;
        const size_t off = ((size_t)(ok ? kq : 0) * BN + (ok ? n : 0)) * 8;      // Npad1 = Npad2 = Npad3 = BN (down_unit_covers)
        const unsigned mk = opaque_mask(ok);
        uint4 vh = *reinterpret_cast<const uint4*>(reinterpret_cast<const h16*>(Wh_) + off), vl = *reinterpret_cast<const uint4*>(reinterpret_cast<const h16*>(Wl_) + off);
        vh.x &= mk; vh.y &= mk; vh.z &= mk; vh.w &= mk; vl.x &= mk; vl.y &= mk; vl.z &= mk; vl.w &= mk;
        bh = *reinterpret_cast<h16x8*>(&vh); bl = *reinterpret_cast<h16x8*>(&vl);
    };
    h16x8 g1h[2], g1l[2], g2h[KS2], g2l[KS2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) frag(a.W1h, a.W1l, ks, KQ1, nt1 * 32 + l31, true, g1h[ks], g1l[ks]);
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {                               // pw2 (K = bf) on wavefronts 0..NP-1, branch 1's pointwise conv (K = cin: two steps) behind them
        const bool use = pw2_wave || (b1_wave && ks < 2);
        frag(pw2_wave ? a.W2h : a.W3h, pw2_wave ? a.W2l : a.W3l, ks, pw2_wave ? KQ2 : KQ1, nt2 * 32 + l31, use, g2h[ks], g2l[ks]);
    }
    const float bias1 = (nt1 * 32 + l31 < bf) ? a.b1[nt1 * 32 + l31] : 0.0f;
    const float bias23 = (nt2 * 32 + l31 < bf && (pw2_wave || b1_wave)) ? (pw2_wave ? a.b2 : a.b3)[nt2 * 32 + l31] : 0.0f;
    // window pieces of this thread: 16-byte piece e = t + 256 i of the WH runs of WW * cin floats; everything about a piece that does not
    // depend on the tile is computed here
    constexpr int QR = WW * cq;
    int wpos[NLD], wrel[NLD];                                        // wy | wx << 8 | first channel << 16 (or -1); offset from the window's first float
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = t + 256 * i;
        const int wy = e / QR, q = e - wy * QR;
        const int wx = q / cq, c4 = (q - wx * cq) * 4;
        wpos[i] = (e < WH * QR) ? (wy | (wx << 8) | (c4 << 16)) : -1;
        wrel[i] = (wy * a.W + wx) * cin + c4;
    }
    float4 pre[NLD];
    unsigned pok = 0;
    const char* xbase = reinterpret_cast<const char*>(a.x);
    auto request = [&](int tile) {
        const int b = tile / per_img, trem = tile - b * per_img;
        const int ty = trem / tx_n, tx = trem - ty * tx_n;
        const int iy0 = 2 * ty * TH - 1, ix0 = 2 * tx * TW - 1;
        const int org = ((b * a.H + iy0) * a.W + ix0) * cin;         // the window's first float (outside the tensor on the image border: never used then)
        pok = 0;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int wy = wpos[i] & 0xff, wx = (wpos[i] >> 8) & 0xff;
            const bool ok = wpos[i] >= 0 && (unsigned)(iy0 + wy) < (unsigned)a.H && (unsigned)(ix0 + wx) < (unsigned)a.W;
            // raw value from a clamped address; zeroed when it is CONSUMED (a mask applied here would wait for the load here)
            pre[i] = *reinterpret_cast<const float4*>(xbase + (unsigned)(ok ? org + wrel[i] : 0) * 4u);
            pok |= (ok ? 1u : 0u) << i;
        }
    };
    request(tbase + tl);
    if (t < RT1 * 32 - NPIX) inside[NPIX + t] = 0;                   // pad rows of the last row tile: never inside
    float amax = 0.0f;                                               // range guard (yn_split.h): largest |value| this thread has split
    float* PT = T32;                                                 // [32][2 bf]: the output tile, both branches shuffled together

    // ---- 1. the window: fp32 copy + split planes; K tail of the planes (run for the NEXT tile in front of the current tile's stores: the wait
    //      for the prefetch must not stand behind them in the memory counter) --------------------------------------------------------
    auto consume = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            if (wpos[i] >= 0) {
                const int wy = wpos[i] & 0xff, wx = (wpos[i] >> 8) & 0xff, c4 = (wpos[i] >> 16) & 0xff;
                const int p = wy * WW + wx;
                const float4 v = vmask(pre[i], 0u - ((pok >> i) & 1u));
                *reinterpret_cast<float4*>(X32 + p * cin + c4) = v;
                const float x4[4] = {v.x, v.y, v.z, v.w};
                h16x4 hi, lo;
#pragma unroll
                for (int j = 0; j < 4; ++j) { amax = range_track(amax, x4[j]); hi[j] = (h16)x4[j]; lo[j] = split_lo(x4[j], hi[j]); }
                *reinterpret_cast<h16x4*>(A1h + p * AST1 + c4) = hi;
                *reinterpret_cast<h16x4*>(A1l + p * AST1 + c4) = lo;
                if (c4 == 0) inside[p] = (unsigned char)((pok >> i) & 1u);
            }
        }
        if constexpr (cin < 32) {
            constexpr int ntail = (32 - cin) >> 2;                   // quads of zero columns up to K = 32
#pragma unroll
            for (int i0 = 0; i0 < RT1 * 32 * ntail; i0 += 256) {
                const int i = i0 + t;
                if (i0 + 256 > RT1 * 32 * ntail && i >= RT1 * 32 * ntail) break;
                const int p = i / ntail, c2 = cin + 4 * (i - p * ntail);
                *reinterpret_cast<uint2*>(A1h + p * AST1 + c2) = make_uint2(0u, 0u);
                *reinterpret_cast<uint2*>(A1l + p * AST1 + c2) = make_uint2(0u, 0u);
            }
        }
    };
    consume();

    for (;;) {
        const int tile = tbase + tl;
        const int b = tile / per_img, trem = tile - b * per_img;
        const int oy0 = (trem / tx_n) * TH, ox0 = (trem % tx_n) * TW;
        __syncthreads();
        YN_TS();
        const bool more = tl + GL < TL && tbase + tl + GL < tiles;
        if (more) request(tbase + tl + GL);                          // the next tile's round trip runs under phases 2-4

        // ---- 2. y1 = act(pw1) on the window pixels -> T32 (zero outside the image) ---------------------------------------------------
        // items it0, it0 + 4, ... of this wavefront (three at most), unrolled: the A fragments and `inside` words of ALL of them are read in front
        // of the first MFMA chain (reads(j + 2) stands in front of chain j).  One accumulator pair: the chain of item j + 1 issued in front of
        // the epilogue of item j measured equal at 16 more registers, and with all reads first it needs scratch.
        // The last item exists on some wavefronts only (a wave-uniform guard); its reads come from a clamped row tile.
        {
            constexpr int NITEMS = RT1 * NP, NFULL = NITEMS / 4, NIT1 = (NITEMS + 3) / 4;
            const bool last_ok = it0 + 4 * NFULL < NITEMS;
            h16x8 fah[NIT1][2], fal[NIT1][2];
            int inw[NIT1][4];                                        // inside flags of this lane's 16 rows: four bytes per word
            auto reads = [&](int j) {
                const int rt = (j < NFULL || last_ok) ? (it0 + 4 * j) / NP : 0;
                const h16* Ahb = A1h + (rt * 32 + l31) * AST1 + h * 8;
                const h16* Alb = A1l + (rt * 32 + l31) * AST1 + h * 8;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    fah[j][ks] = *reinterpret_cast<const h16x8*>(Ahb + ks * 16);
                    fal[j][ks] = *reinterpret_cast<const h16x8*>(Alb + ks * 16);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) inw[j][g] = *reinterpret_cast<const int*>(inside + rt * 32 + 8 * g + 4 * h);
            };
            reads(0);
            if (NIT1 > 1) reads(1);
#pragma unroll
            for (int j = 0; j < NIT1; ++j) {
                if (j + 2 < NIT1) reads(j + 2);
                if (j < NFULL || last_ok) {
                    f32x16 acc0, acc1;
#pragma unroll
                    for (int k = 0; k < 16; ++k) { acc0[k] = 0.0f; acc1[k] = 0.0f; }
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) split_mfma(fah[j][ks], fal[j][ks], &g1h[ks], &g1l[ks], acc0, acc1);
                    const int rt = (it0 + 4 * j) / NP;
                    const int n = nt1 * 32 + l31;
                    if (n < bf) {
                        float* trow = T32 + (rt * 32 + 4 * h) * CS + n;  // row (r & 3) + 8 (r >> 2) of this lane's half: a wave-uniform offset
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = act_pw(split_join(acc0[r], acc1[r]) + bias1, a.act1);
                            trow[((r & 3) + 8 * (r >> 2)) * CS] = __uint_as_float(__float_as_uint(v) & (unsigned)__builtin_amdgcn_sbfe(inw[j][r >> 2], 8 * (r & 3), 1));
                        }
                    }
                }
            }
        }
        __syncthreads();                                             // y1 complete; the A1 planes are free
        YN_TS();

        // ---- 3. both depthwise convs (stride 2, dwconv3x3_kernel's fma chain) -> the split planes of their branch --------------------
        {                                                            // the window reads of all of a thread's outputs first, then their fma chains side by side
            float2 xv[NI1][9], acc[NI1];
#pragma unroll
            for (int i = 0; i < NI1; ++i) {
                const int op = p1 + i * p1_n, opc = op < NO ? op : 0;
                const int dy = opc / TW, dx = opc - dy * TW;
                const float* xw = X32 + (2 * dy * WW + 2 * dx) * cin + c1;
#pragma unroll
                for (int k = 0; k < 9; ++k) xv[i][k] = *reinterpret_cast<const float2*>(xw + ((k / 3) * WW + k % 3) * cin);
                acc[i] = b1d;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int i = 0; i < NI1; ++i) vfma(acc[i], xv[i][k], w1d[k]);
#pragma unroll
            for (int i = 0; i < NI1; ++i) {
                const int op = p1 + i * p1_n;
                if (p1 < p1_n && op < NO) {
                    if (!RELU) acc[i] = vact(acc[i], a.dw1_act);
                    amax = range_track(range_track(amax, acc[i].x), acc[i].y);
                    h16x2 hi, lo;
                    hi[0] = (h16)acc[i].x; hi[1] = (h16)acc[i].y;
                    lo[0] = split_lo(acc[i].x, hi[0]); lo[1] = split_lo(acc[i].y, hi[1]);
                    *reinterpret_cast<h16x2*>(A3h + op * AST1 + c1) = hi;
                    *reinterpret_cast<h16x2*>(A3l + op * AST1 + c1) = lo;
                }
            }
        }
        {
            constexpr int pad1 = (AST1 - cin) >> 2;                    // K tail of branch 1's planes: zero (quads: cin is a multiple of 4)
#pragma unroll
            for (int i0 = 0; i0 < NO * pad1; i0 += 256) {
                const int i = i0 + t;
                if (i0 + 256 > NO * pad1 && i >= NO * pad1) break;
                const int r = i / pad1, c2 = cin + 4 * (i - r * pad1);
                *reinterpret_cast<uint2*>(A3h + r * AST1 + c2) = make_uint2(0u, 0u);
                *reinterpret_cast<uint2*>(A3l + r * AST1 + c2) = make_uint2(0u, 0u);
            }
        }
        {
            float2 yv[NI2][9], acc[NI2];
#pragma unroll
            for (int i = 0; i < NI2; ++i) {
                const int op = dpl + i * ppl, opc = op < NO ? op : 0;
                const int dy = opc / TW, dx = opc - dy * TW;
                const float* yw = T32 + (2 * dy * WW + 2 * dx) * CS + dc;
#pragma unroll
                for (int k = 0; k < 9; ++k) yv[i][k] = *reinterpret_cast<const float2*>(yw + ((k / 3) * WW + k % 3) * CS);
                acc[i] = bd;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int i = 0; i < NI2; ++i) vfma(acc[i], yv[i][k], wd[k]);
#pragma unroll
            for (int i = 0; i < NI2; ++i) {
                const int op = dpl + i * ppl;
                if (dworker && op < NO) {
                    if (!RELU) acc[i] = vact(acc[i], a.dw_act);
                    amax = range_track(range_track(amax, acc[i].x), acc[i].y);
                    h16x2 hi, lo;
                    hi[0] = (h16)acc[i].x; hi[1] = (h16)acc[i].y;
                    lo[0] = split_lo(acc[i].x, hi[0]); lo[1] = split_lo(acc[i].y, hi[1]);
                    *reinterpret_cast<h16x2*>(A2h + op * AST2 + dc) = hi;
                    *reinterpret_cast<h16x2*>(A2l + op * AST2 + dc) = lo;
                }
            }
        }
        {
            constexpr int padn = (AST2 - bf) >> 1;                     // K tail of both planes: zero (pairs: bf is even)
#pragma unroll
            for (int i0 = 0; i0 < NO * padn; i0 += 256) {
                const int i = i0 + t;
                if (i0 + 256 > NO * padn && i >= NO * padn) break;
                const int r = i / padn, c2 = bf + 2 * (i - r * padn);
                *reinterpret_cast<unsigned*>(A2h + r * AST2 + c2) = 0u;
                *reinterpret_cast<unsigned*>(A2l + r * AST2 + c2) = 0u;
            }
        }
        __syncthreads();
        YN_TS();

        // ---- 4. branch 1's pointwise conv on wavefronts NP..2NP-1 while wavefronts 0..NP-1 run pw2; both -> PT, in the free T32 space -----
        f32x16 acc0, acc1;
#pragma unroll
        for (int k = 0; k < 16; ++k) { acc0[k] = 0.0f; acc1[k] = 0.0f; }
        constexpr int PS = 2 * bf;                                   // PT: [32 tile pixels][2 bf] in the output's own shuffled order - a tile row is ONE contiguous run of it
        if (b1_wave) {
            const h16* Ahb = A3h + l31 * AST1 + h * 8;
            const h16* Alb = A3l + l31 * AST1 + h * 8;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const h16x8 ah = *reinterpret_cast<const h16x8*>(Ahb + ks * 16);
                const h16x8 al = *reinterpret_cast<const h16x8*>(Alb + ks * 16);
                split_mfma(ah, al, &g2h[ks], &g2l[ks], acc0, acc1);
            }
        }
        if (pw2_wave) {                                              // pw2: one wavefront per 32 output columns, gemm_split_tile's chunks of 32 (whole chunks, zero-padded)
            const h16* Ahb = A2h + l31 * AST2 + h * 8;
            const h16* Alb = A2l + l31 * AST2 + h * 8;
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                const h16x8 ah = *reinterpret_cast<const h16x8*>(Ahb + ks * 16);
                const h16x8 al = *reinterpret_cast<const h16x8*>(Alb + ks * 16);
                split_mfma(ah, al, &g2h[ks], &g2l[ks], acc0, acc1);
            }
        }
        // concat + shuffle in LDS: column 2n = branch 1, 2n + 1 = branch 2.  Row r of the accumulator = tile pixel (r >> 2, (r & 3) + 4 h)
        if ((pw2_wave || b1_wave) && nt2 * 32 + l31 < bf) {
            float* prow = PT + (4 * h) * PS + 2 * (nt2 * 32 + l31) + (pw2_wave ? 1 : 0);
            const int act23 = pw2_wave ? a.act2 : a.act3;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                prow[((r & 3) + 8 * (r >> 2)) * PS] = act_pw(split_join(acc0[r], acc1[r]) + bias23, act23);
        }
        __syncthreads();                                             // the output tile is complete; nobody reads the planes, the fp32 window or the flags any more
        if (more) consume();                                         // the next tile's window -> LDS (PT, which the store below reads, lies in T32)
        // ---- 5. the store, by all four wavefronts: the 16-byte pieces of the tile's rows (8 pixels x 2 bf floats: contiguous in `out` and in PT) ----
        {
            // byte offsets in 32 bits (down_unit_covers: the output tensor is below 4 GB): ONE 64-bit base, the kernel argument itself
            char* obase = reinterpret_cast<char*>(a.out);
            const unsigned tile_off = (unsigned)(((b * Ho + oy0) * Wo + ox0) * 2 * bf) * 4u;
            constexpr int PQ = bf / 2, RQ = TW * PQ, NST = (TH * RQ + 255) / 256;      // pieces per pixel, per tile row, per thread
            float4 ov[NST];
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int e = t + 256 * i;
                ov[i] = *reinterpret_cast<const float4*>(PT + (e < TH * RQ ? e : 0) * 4);
            }
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int e = t + 256 * i;
                const int dy = e / RQ, q = e - dy * RQ, dx = q / PQ;
                if (e < TH * RQ && oy0 + dy < Ho && ox0 + dx < Wo)
                    *reinterpret_cast<float4*>(obase + (tile_off + (unsigned)(dy * Wo * 2 * bf) * 4u + (unsigned)q * 16u)) = ov[i];
            }
        }
        YN_TS();
        if (!more) break;
        tl += GL;
    }
    range_report(a.ovf, amax);
#ifdef YN_EXP_TIMING
    if (t == 0 && (blockIdx.x % 61) == 7 && tsn >= 5)
        printf("downpipe blk %d invariants+window %lld gemm1 %lld dw %lld gemm2+store %lld first tile %lld second %lld\n", (int)blockIdx.x, TS[1] - TS[0], TS[2] - TS[1], TS[3] - TS[2],
               TS[4] - TS[3], TS[4] - TS[0], tsn >= 8 ? TS[7] - TS[4] : -1LL);
#endif
#undef YN_TS
}

static size_t down_unit_pipe_lds(int bf, int cin)
{
    return ((size_t)160 * 40 + (size_t)160 * cin + (size_t)160 * (bf + 2)) * sizeof(float) + 160;
}

// what down_unit_pipe_kernel takes: exactly the widths it is instantiated for - (cin, bf) = (24, 58) at 1.0x and (24, 24) at 0.5x; wider stages take
// the down2 path - with one column block per GEMM, even maps and 32-bit byte offsets
bool down_unit_covers(const DownArgs& a)
{
    const bool widths = a.cin == 24 && (a.bf == 58 || a.bf == 24);
    return widths && a.W1h && a.W1l && a.W2h && a.W2l && a.Npad1 == a.Npad2 && a.Npad1 == 32 * ((a.bf + 31) / 32) &&
           !(a.H & 1) && !(a.W & 1) && a.B > 0 && (size_t)a.B * a.H * a.W * (size_t)(a.cin > a.bf / 2 ? a.cin : a.bf / 2) < ((size_t)1 << 30) &&      // 32-bit byte offsets
           a.wdw1 && a.bdw1 && a.W3h && a.W3l && a.b3 && a.Npad3 == a.Npad1;
}

void launch_down_unit(const DownArgs& a, hipStream_t s)
{
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    const unsigned tiles = (unsigned)a.B * ((Ho + 3) / 4) * ((Wo + 7) / 8);
    static unsigned long long attr = 0;
    if (attr_pending(attr)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down_unit_pipe_kernel<24, 24, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down_unit_pipe_kernel<24, 58, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down_unit_pipe_kernel<24, 24, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down_unit_pipe_kernel<24, 58, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    constexpr unsigned pipe_g = 1024;   // walking workgroups (a multiple of 8): ~3 tiles each at bs = 32 (512 / 768 / 1024 / 1456 / one per tile measured within 1 % of each other)
    const size_t plds = down_unit_pipe_lds(a.bf, a.cin);
    unsigned g = xcd_grid(tiles);
    if (g > pipe_g) g = pipe_g;
    const bool relu = a.act1 == 1 && a.act2 == 1 && a.act3 == 1 && a.dw_act == 0 && a.dw1_act == 0;
#define YN_DUP(ci, bw, rl) { set_last_kernel_name("down_unit_pipe_kernel<" #ci "," #bw "," #rl ">"); hipLaunchKernelGGL((down_unit_pipe_kernel<ci, bw, rl>), dim3(g), dim3(256), plds, s, a, (int)tiles); }
    if (a.bf == 24) { if (relu) YN_DUP(24, 24, true) else YN_DUP(24, 24, false) }
    else            { if (relu) YN_DUP(24, 58, true) else YN_DUP(24, 58, false) }
#undef YN_DUP
}

// -------------------------------------------------------------------------------------------------
// The stride-2 ShuffleV2 units of stages 3 and 4 (backbone/shufflenetv2.py:42-49, 53-63, 73-74; cin = bf = 116 / 232): too wide for
// down_unit_pipe_kernel's window form (pw1 on the 17 x 9 halo needs the whole K = cin of 153 pixels in LDS).  The unit is cut where the chain
// kernels cut theirs - at the depthwise convs, after which everything is pixel-local:
//     launch 1 (gemm_split_kernel):  y1 = relu(pw1(x))                                          [B][H][W][bf]
//     launch 2 (down2_kernel):       y3 = relu(pw2(dw_s2(y1))),  z2 = relu(pw(dw_s2(x))),  out = shuffle(cat(z2, y3))
// Two launches instead of five; the four tensors between them (both depthwise outputs, branch 1's output, 60 MB per step at stage 3)
// never reach memory.  Workgroup = 32 consecutive output pixels (flat, all images): thread = (4 channels, every ppl-th pixel) with the
// nine taps of its channels in registers; the 3 x 3 stride-2 windows of TWO pixels are in flight per round (18 clamped, masked 16-byte
// loads), results split straight into the A planes of their branch; then ONE chunk loop walks the K chunks of pw2 and of branch 1's
// pointwise conv back to back (the next chunk's weights always in flight), four wavefronts x NT column tiles.  The accumulator layout
// gives a lane the SAME column n and the same 16 rows in both GEMMs, so the concat + shuffle is the store: out[row][2n .. 2n+1] =
// (z2, y3) as one 8-byte store.  Every sum in the order of dwconv3x3_kernel / gemm_split_kernel: bit-identical to the five launches
// (test_down_unit_is_bit_identical).  LDS 48 KB at bf = 116 (three workgroups per CU: the 676 workgroups of a 32-image step are all resident).
// -------------------------------------------------------------------------------------------------
template <int NT, int D>                                   // NT column tiles of 32 per wavefront (4 wavefronts); D k-steps of weights in flight
__global__ __launch_bounds__(256, NT == 1 ? 3 : 1) void down2_kernel(Down2Args a)
{
    constexpr int BM = 32;
    extern __shared__ __attribute__((aligned(16))) float d2_smem[];
    const int bf = a.bf, cin = a.cin;
    const int KQ2 = (bf + 7) >> 3, KQ1 = (cin + 7) >> 3, PS2 = plane_stride(bf), PS1 = plane_stride(cin);
    const int S2 = (KQ2 + 1) >> 1, S1 = (KQ1 + 1) >> 1, S = S2 + S1;    // 16-deep k-steps of pw2, of branch 1's pointwise conv
    const bool chain = a.W1nh != nullptr;                               // + the next unit's pw1 (K = bf: S2 steps more, after the store)
    h16* A2h = reinterpret_cast<h16*>(d2_smem);                     // [BM][PS2]
    h16* A2l = A2h + BM * PS2;
    h16* A1h = A2l + BM * PS2;                                        // [BM][PS1]
    h16* A1l = A1h + BM * PS1;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1, HWo = Ho * Wo, Mo = a.B * HWo;
    const int m0 = (int)xcd_block(blockIdx.x, gridDim.x) * BM;
    if (m0 >= Mo) return;
    const int nrows = Mo - m0 < BM ? Mo - m0 : BM;

#ifdef YN_EXP_TIMING
    long long TS[8]; int tsn = 0;
#define YN_TS() TS[tsn++] = __builtin_readcyclecounter()
#else
#define YN_TS()
#endif
    YN_TS();
    // The weights never pass through LDS: a lane's B fragment of a k-step is 16 contiguous bytes of the pre-split pack
    // ([octet][column][8 halves]; the 32 lanes of a half-wavefront read 512 contiguous bytes), so every wavefront streams the fragments of
    // ITS columns straight from L2 into registers, D k-steps ahead, with no barrier between the steps of the two pointwise convs (the first
    // form staged K chunks through LDS: eight barrier rounds of ~3.7 k cycles, each waiting for a load issued one round earlier behind the
    // other workgroups' window traffic - 30 k of the workgroup's 60 k cycles).  Step s of the walk: pw2's steps, then branch 1's.
    // The walk is laid out in PADDED steps: every GEMM starts at a multiple of D (G2 = S2 rounded up, G1 likewise), so that the unrolled
    // D-step body holds nothing but loads, two LDS reads and MFMAs, and what happens between the GEMMs stands once, between the loops (it
    // stood inside every unrolled step, D copies of the store epilogue: a 50-100 KB loop body the instruction cache could not hold - a k-step
    // cost ~900 cycles for 192 cycles of MFMAs even with six workgroups on an idle chip).  A padded step multiplies the zero K tail: exact zeros.
    const int G2 = (S2 + D - 1) / D * D, G1 = (S1 + D - 1) / D * D;
    h16x8 bq[D][NT][2];
    auto load_b = [&](int s, h16x8 (&dst)[NT][2]) {          // s: padded step
        const bool second = s >= G2, third = s >= G2 + G1;
        const int ks = third ? s - (G2 + G1) : (second ? s - G2 : s), KQ = (second && !third) ? KQ1 : KQ2;
        // (without a next unit the steps >= S are masked loads at a clamped address: the base must still be a real pointer)
        const h16* Wh = reinterpret_cast<const h16*>((third && chain) ? a.W1nh : ((second && !third) ? a.W3h : a.W2h));
        const h16* Wl = reinterpret_cast<const h16*>((third && chain) ? a.W1nl : ((second && !third) ? a.W3l : a.W2l));
        // no masks (unit_chain2_kernel's load_b: a masked load is waited for where it is issued - the walk then paid a memory round trip per
        // k-step): clamped octet / column, and the steps past the walk take their A fragment from the planes' zero K tail
        const int kq = min(ks * 2 + h, KQ - 1);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = min((wave * NT + nt) * 32 + l31, a.Npad - 1);
            const size_t off = ((size_t)kq * a.Npad + n) * 8;
            dst[nt][0] = *reinterpret_cast<const h16x8*>(Wh + off);
            dst[nt][1] = *reinterpret_cast<const h16x8*>(Wl + off);
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) load_b(j, bq[j]);                        // requested first: they return before the window loads below
    // ---- 1. both depthwise convs (stride 2, dwconv3x3_kernel's fma chain) -> the split planes of their branch ---------------------------
    float amax = 0.0f;                                                   // range guard (yn_split.h)
    auto dw_branch = [&](const float* __restrict__ src, int C, const float* __restrict__ wd, const float* __restrict__ bd, int act, h16* Ph, h16* Pl, int PS) {
        const int cqn = C >> 2, ppl = 256 / cqn;
        const int cq = t % cqn, pl = t / cqn, c = cq * 4;
        if (pl < ppl) {
            float4 w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const float4*>(wd + k * C + c);
            const float4 bias = *reinterpret_cast<const float4*>(bd + c);
            for (int r0 = pl; r0 < nrows; r0 += 2 * ppl) {
                float4 win[2][9];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int r = r0 + u * ppl;
                    const int m = m0 + (r < nrows ? r : r0);
                    const int b = m / HWo, rem = m - b * HWo;
                    const int oy = rem / Wo, ox = rem - oy * Wo;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int iy = 2 * oy - 1 + ky;
                        const bool yok = iy >= 0 && iy < a.H;
                        const float* rowp = src + ((size_t)(b * a.H + (yok ? iy : 0)) * a.W) * C + c;
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const int ix = 2 * ox - 1 + kx;
                            const bool ok = yok && ix >= 0 && ix < a.W;
                            win[u][ky * 3 + kx] = vmask(*reinterpret_cast<const float4*>(rowp + (size_t)(ok ? ix : 0) * C), opaque_mask(ok));
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int r = r0 + u * ppl;
                    if (r < nrows) {
                        float4 acc = bias;
#pragma unroll
                        for (int k = 0; k < 9; ++k) vfma(acc, win[u][k], w[k]);
                        acc = vact(acc, act);
                        const float x4[4] = {acc.x, acc.y, acc.z, acc.w};
                        h16x4 hi, lo;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { amax = range_track(amax, x4[j]); hi[j] = (h16)x4[j]; lo[j] = split_lo(x4[j], hi[j]); }
                        *reinterpret_cast<h16x4*>(Ph + r * PS + c) = hi;
                        *reinterpret_cast<h16x4*>(Pl + r * PS + c) = lo;
                    }
                }
            }
        }
        // K tail [C, PS) of every row and the idle rows [nrows, BM): zeros (they meet zero weight rows / are never stored, but must not be NaN bit patterns)
        const int padn = PS - C;
        for (int i = t; i < BM * padn; i += 256) { const int r = i / padn, c2 = C + i - r * padn; Ph[r * PS + c2] = (h16)0.0f; Pl[r * PS + c2] = (h16)0.0f; }
        for (int i = t; i < (BM - nrows) * (C >> 2); i += 256) {
            const int r = nrows + i / (C >> 2), c2 = (i % (C >> 2)) * 4;
            h16x4 z; z[0] = z[1] = z[2] = z[3] = (h16)0.0f;
            *reinterpret_cast<h16x4*>(Ph + r * PS + c2) = z; *reinterpret_cast<h16x4*>(Pl + r * PS + c2) = z;
        }
    };
    dw_branch(a.y1, bf, a.wdw, a.bdw, a.dw_act, A2h, A2l, PS2);
    YN_TS();
    dw_branch(a.x, cin, a.wdw1, a.bdw1, a.dw1_act, A1h, A1l, PS1);
    YN_TS();
    // the biases of this lane's columns: requested here (not live during the register-hungry window rounds), used thousands of cycles later
    float bias2[NT], bias3[NT], bias1n[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = (wave * NT + nt) * 32 + l31;
        bias2[nt] = n < bf ? a.b2[n] : 0.0f;
        bias3[nt] = n < bf ? a.b3[n] : 0.0f;
        bias1n[nt] = (chain && n < bf) ? a.b1n[n] : 0.0f;
    }
    __syncthreads();                                                    // both operand tiles are complete
    YN_TS();
    range_report(a.ovf, amax);                                          // every split of this workgroup is done

    // ---- 2. the pointwise convs as ONE walk over their k-steps (gemm_split_tile's order inside each): pw2, branch 1's, then - with a next
    //      unit behind this one - that unit's pw1, whose operand is produced half way (step S): the weight fragments keep streaming across
    //      the two barriers there ---------------------------------------------------------------------------------------------------------
    f32x16 acc0[NT], acc1[NT];
    float y3[NT][16];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) { acc0[i][k] = 0.0f; acc1[i][k] = 0.0f; }
    const int jhi = bf >> 1;
    char* out_base = reinterpret_cast<char*>(a.out + (size_t)m0 * (2 * bf));
    // concat + shuffle store: out[row][2n] = branch 1, out[row][2n + 1] = branch 2; with a next unit behind it, the pairs of the columns
    // n >= bf/2 - channels [bf, 2bf) of the output: that unit's x2 - are ALSO split into the (then free) planes of branch 2
    auto store_pairs = [&]() {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = (wave * NT + nt) * 32 + l31;
            if (n < bf) {
                const bool to_plane = chain && n >= jhi;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float z = apply_act(split_join(acc0[nt][r], acc1[nt][r]) + bias3[nt], a.act3);
                    if (row < nrows) *reinterpret_cast<float2*>(out_base + (unsigned)(row * 2 * bf + 2 * n) * 4u) = make_float2(z, y3[nt][r]);
                    if (to_plane) {                                     // (idle rows carry finite values of zero operands: never stored)
                        const float v0 = z, v1 = y3[nt][r];
                        h16x2 hi, lo;
                        amax = range_track(range_track(amax, v0), v1);
                        hi[0] = (h16)v0; hi[1] = (h16)v1;
                        lo[0] = split_lo(v0, hi[0]); lo[1] = split_lo(v1, hi[1]);
                        *reinterpret_cast<h16x2*>(A2h + row * PS2 + 2 * (n - jhi)) = hi;
                        *reinterpret_cast<h16x2*>(A2l + row * PS2 + 2 * (n - jhi)) = lo;
                    }
                }
            }
        }
    };
    auto run_gemm = [&](const h16* Ah_, const h16* Al_, int PS, int Sn, int p0, int p1) {     // padded steps [p0, p1) of one GEMM (Sn real k-steps)
        const h16* ahp = Ah_ + l31 * PS + h * 8;
        const h16* alp = Al_ + l31 * PS + h * 8;
        for (int s0 = p0; s0 < p1; s0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int ks = s0 + j - p0;
                const int a_col = ks < Sn ? ks * 16 : PS - 8 - h * 8;  // padded step: the last 16 bytes of the row's zero K tail
                const h16x8 ah = *reinterpret_cast<const h16x8*>(ahp + a_col);
                const h16x8 al = *reinterpret_cast<const h16x8*>(alp + a_col);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    split_mfma(ah, al, bq[j][nt][0], bq[j][nt][1], acc0[nt], acc1[nt]);
                }
                load_b(s0 + j + D, bq[j]);                              // (clamped beyond the walk)
            }
        }
    };
    run_gemm(A2h, A2l, PS2, S2, 0, G2);                                 // pw2: its tile then waits in registers for its partner
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            y3[nt][r] = apply_act(split_join(acc0[nt][r], acc1[nt][r]) + bias2[nt], a.act2);
            acc0[nt][r] = 0.0f; acc1[nt][r] = 0.0f;
        }
    run_gemm(A1h, A1l, PS1, S1, G2, G2 + G1);                           // branch 1's pointwise conv
    if (chain) {                                                        // the unit's output is complete: store it, x2' -> planes, the next unit's pw1
        __syncthreads();                                                // every wavefront is past its last read of the planes
        store_pairs();
        __syncthreads();                                                // x2' is complete (its K tail [bf, PS2) is still zero)
        range_report(a.ovf, amax);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[nt][r] = 0.0f; acc1[nt][r] = 0.0f; }
        run_gemm(A2h, A2l, PS2, S2, G2 + G1, G2 + G1 + G2);
    }
    YN_TS();
    if (!chain) {
        store_pairs();
    } else {
        // the next unit's pw1 -> t1n (gemm_split_kernel's epilogue: 16-byte stores through the in-quad transpose)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) split_join(acc0[nt], acc1[nt]);
        GemmArgs e{};
        e.out = a.t1n; e.out_ld = bf; e.out_off = 0; e.M = m0 + nrows; e.N = bf; e.Npad = a.Npad; e.bias = a.b1n; e.act = a.act1n; e.pass = nullptr;
        gemm_epilogue<NT>(e, acc0, m0, wave * NT * 32, true, lane, bias1n);
    }
#ifdef YN_EXP_TIMING
    YN_TS();
    if (t == 0 && (blockIdx.x % 97) == 5)
        printf("down2 bf %d blk %d dw2 %lld dw1 %lld sync %lld walk %lld end %lld total %lld\n", bf, (int)blockIdx.x, TS[1] - TS[0], TS[2] - TS[1], TS[3] - TS[2],
               TS[4] - TS[3], TS[5] - TS[4], TS[5] - TS[0]);
#endif
#undef YN_TS
}

static size_t down2_lds(int bf, int cin)
{
    const int PS2 = plane_stride(bf), PS1 = plane_stride(cin);
    return ((size_t)2 * 32 * PS2 + (size_t)2 * 32 * PS1) * 2;
}

bool down2_covers(const Down2Args& a)
{
    return a.x && a.y1 && a.W2h && a.W2l && a.W3h && a.W3l && a.wdw && a.wdw1 && a.bdw && a.bdw1 && a.b2 && a.b3 && a.B > 0 && a.H > 1 && a.W > 1 &&
           a.bf >= 4 && a.cin >= 4 && !(a.bf & 3) && !(a.cin & 3) && a.bf <= 256 && a.cin <= 256 && a.Npad >= a.bf && a.Npad <= 256 &&
           (long)a.B * a.H * a.W * (a.bf > a.cin ? a.bf : a.cin) < (1l << 30);
}

void launch_down2(const Down2Args& a, hipStream_t s)
{
    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1;
    const unsigned tiles = (unsigned)(((long)a.B * Ho * Wo + 31) / 32);
    static unsigned long long attr = 0;
    if (attr_pending(attr)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down2_kernel<1, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(down2_kernel<2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    if (a.Npad <= 128) { set_last_kernel_name("down2_kernel<1,4>"); hipLaunchKernelGGL((down2_kernel<1, 4>), dim3(xcd_grid(tiles)), dim3(256), down2_lds(a.bf, a.cin), s, a); }
    else               { set_last_kernel_name("down2_kernel<2,4>"); hipLaunchKernelGGL((down2_kernel<2, 4>), dim3(xcd_grid(tiles)), dim3(256), down2_lds(a.bf, a.cin), s, a); }
}

// -------------------------------------------------------------------------------------------------
// Depthwise 3x3 + pointwise conv of a detection head (models/yolo_nano.py:60-82: Conv(96, 96, k=3, g=96) -> Conv(96, 96, k=1)) as one
// kernel, for up to three pyramid levels per launch (Group<>).  The depthwise output of the stride-8 head is 33 MB per 32-image step,
// written by one launch and read back by the next; here it goes from registers into the GEMM's LDS operand planes.  One tile = 8 x 4
// pixels of one image; 192 threads = three wavefronts = the three 32-column tiles of the GEMM, 16-byte stores through the in-quad
// transpose.  The 96 x 96 split weights are register-resident (a lane's B fragments of its wavefront's 32 columns: 48 registers, loaded
// once per workgroup - nothing of them in LDS).
//
// A PERSISTENT, software-pipelined walk after unit_pipe_kernel (kernels_pipe.hip):
//   * a tile's depthwise window - six row runs of ten pixels x 96 channels, 3 840 contiguous bytes of the NHWC input each - arrives in LDS
//     by LDS-DMA (dma16: no registers, no staging instructions): a row run is four pieces of 1 KB (240 granules of a pixel's channel quad +
//     16 of padding, which fetch the last granule again), wavefront w brings rows 2 w and 2 w + 1 - eight pieces per wavefront and tile,
//     each at a wave-uniform LDS base AND from a wave-uniform global row: the row's clamped start is scalar arithmetic, a lane's place in
//     the row is the same in both rows - four lane offsets per tile, no vector instruction per piece.  Rows and pixels outside the image
//     are fetched from the clamped address (LDS-DMA cannot write zeros) and zeroed where they are consumed (`wok` / vmask, as the register
//     form did);
//   * ONE window buffer, 168 registers, 37 KB of LDS: FOUR workgroups per CU, three wavefronts on every SIMD (the register form: 222 registers,
//     two workgroups, six wavefronts on four SIMDs).  The window of tile n + 1 is requested right behind the barrier that ends tile n's
//     depthwise phase - the buffer's last reader - and flies under the GEMM and the epilogue's arithmetic; each wavefront waits for its own
//     pieces in front of its stores (nothing else is in flight there but the previous tile's stores, a whole tile old), and the barrier
//     that ends the tile orders every wavefront's pieces before the reads (wait, barrier, read: MI355X orders an LDS read behind a DMA
//     piece by nothing else).  What covers the rest of the round trip is the other three workgroups of the CU.  The form with two window
//     buffers, requested two tiles ahead behind a counted s_waitcnt vmcnt(8), fits two workgroups per CU and measured slower;
//   * the depthwise conv reads its 3 x 6 window row by row with 16-byte LDS reads (consecutive lanes = consecutive channel quads), thread =
//     (channel quad, run of four pixels along x), the fma chain of dwconv3x3_kernel per output: bias, then ky, kx in order; a tile whose
//     window lies inside the image runs it without the masks;
//   * the grid is what is resident (launch_dwpw_group): the weight panel and the taps are loaded once per slot.
// Bit-identical to dwconv3x3_kernel + gemm_split_kernel (test_grouped_launches_are_bit_identical, tests/test_gpu_dwpw_pipe.py).
// -------------------------------------------------------------------------------------------------
constexpr int DWPW_PLANES = 2 * 32 * 104 * 2;               // the two operand planes [32][96 + 8] of f16
constexpr int DWPW_WIN = 24 * 1024;                         // one window buffer: 6 row runs of four 1 KB pieces (10 pixels x 384 bytes + 256 of padding)
constexpr int DWPW_LDS = DWPW_PLANES + DWPW_WIN;            // 37 888 bytes: four workgroups per CU
constexpr unsigned DWPW_SLOTS = 1024;                       // resident workgroups: 256 CUs x 4 (168 registers: tests/test_isa_dwpw_cpu.py)

__device__ __forceinline__ void dwpw_pipe_block(const DwPwArgs& a, unsigned char* smem, unsigned bid, unsigned nblocks)
{
    constexpr int TW = 8, TH = 4, NO = TW * TH, C = 96, KQ = C / 8, KS = KQ / 2, AST = C + 8, R = 4;
    constexpr int WW = TW + 2, WR = TH + 2, CQ = C / 4, NP = 8;         // window: WR row runs of WW pixels of CQ quads; pieces per wavefront and tile
    constexpr unsigned WROW = 4096;                                     // a row run in LDS: four pieces (3 840 bytes + 256 of padding)
    static_assert(2 * NO * AST * 2 == DWPW_PLANES && WR * WROW == DWPW_WIN && WW * CQ * 16 <= WROW && 3 * NP == 4 * WR, "LDS carve; three wavefronts x two rows");
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    h16* Ah = reinterpret_cast<h16*>(smem);               // [NO][AST]
    h16* Al = Ah + NO * AST;
    const unsigned char* win = smem + DWPW_PLANES;          // [WR rows of WROW bytes]: [WW pixels][CQ] x 16 bytes of fp32
    const unsigned lds_win = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem + (unsigned)DWPW_PLANES;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), l31 = lane & 31, h = lane >> 5;
    const int tx_n = (a.W + TW - 1) / TW, ty_n = (a.H + TH - 1) / TH, per_img = tx_n * ty_n;
    const int tiles = a.B * per_img;
    // XCD-contiguous walk: XCD x (= bid % 8) owns tiles [x TL, (x + 1) TL), its workgroups take them round-robin
    const int TL = (tiles + 7) >> 3, GL = (int)(nblocks >> 3);
    const int tend = ((int)(bid & 7u) + 1) * TL < tiles ? ((int)(bid & 7u) + 1) * TL : tiles;
    const int tile0 = (int)(bid & 7u) * TL + (int)(bid >> 3);
    if (tile0 >= tend) return;                              // no tile: nothing requested

    const int cq = t % CQ, run = t / CQ;                    // 24 channel quads x 8 runs of 4 pixels (2 per tile row) = 192 workers
    const int c = cq * 4, ry = run >> 1, rx = (run & 1) * R;
    // a tile index -> (image, first row, first column), once per tile and wave-uniform
    struct Pos { int b, oy0, ox0; };
    auto decode = [&](int tile) {
        const int b = tile / per_img, trem = tile - b * per_img, ty = trem / tx_n;
        return Pos{__builtin_amdgcn_readfirstlane(b), __builtin_amdgcn_readfirstlane(ty * TH), __builtin_amdgcn_readfirstlane((trem - ty * tx_n) * TW)};
    };
    // the window of one tile -> LDS: eight pieces per wavefront.  Wavefront w brings window rows 2 w and 2 w + 1, four pieces each: the row is
    // wave-uniform - its clamped start goes into the piece's scalar base - and a lane's place in the row, (pixel, quad) of granule
    // 64 k + lane, is the same in both rows: four lane offsets per tile, no vector work per piece
    auto issue = [&](const Pos& p) {
        int tt = t;                                         // (opaque: as loop invariants the four granule decodes are held in registers across the GEMM)
        asm volatile("" : "+v"(tt));
        const int ln = tt & 63;
        unsigned xo[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q = ln + 64 * k;                            // the row's padding granules fetch its last one again
            if (k == 3) q = q < WW * CQ - 1 ? q : WW * CQ - 1;
            const int px = q / CQ, qq = q - px * CQ;
            int ix = p.ox0 - 1 + px;
            ix = ix < 0 ? 0 : (ix < a.W ? ix : a.W - 1);
            xo[k] = (unsigned)(ix * C + qq * 4) * 4u;
        }
        const unsigned dst = lds_win + (unsigned)wave * (2u * WROW);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int iy = p.oy0 - 1 + 2 * wave + (i >> 2);
            iy = iy < 0 ? 0 : (iy < a.H ? iy : a.H - 1);
            const unsigned row = (unsigned)((p.b * a.H + iy) * a.W) * (unsigned)(C * 4);
            dma16(reinterpret_cast<const char*>(a.in) + row, xo[i & 3], dst + (unsigned)(i >> 2) * WROW + (unsigned)(i & 3) * 1024u);
        }
    };
    int t1 = tile0 + GL < tend ? tile0 + GL : -1;           // the next tile of the walk
    Pos cur = decode(tile0), nxt = cur;
    issue(cur);

    // ---- loop invariants: the thread's depthwise taps and bias, the B fragments and bias of its GEMM columns --------------------------
    f32x4 wd[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k] = *reinterpret_cast<const f32x4*>(a.wdw + k * C + c);
    f32x4 bd = *reinterpret_cast<const f32x4*>(a.bdw + c);
    h16x8 gh[KS], gl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const size_t off = ((size_t)(ks * 2 + h) * a.Npad + wave * 32 + l31) * 8;
        gh[ks] = *reinterpret_cast<const h16x8*>(reinterpret_cast<const h16*>(a.Wh) + off);
        gl[ks] = *reinterpret_cast<const h16x8*>(reinterpret_cast<const h16*>(a.Wl) + off);
    }
    float gbias = a.bias[wave * 32 + l31];
    // The first window and the invariants have landed, and hipcc is TOLD so (an asm that reads and writes their registers: its own waits for these
    // loads go HERE, ahead of the loop, not in front of their first use inside it, where a vmcnt(0) would retire the pieces in flight)
    static_assert(KS == 6, "23 asm operands");
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(wd[0]), "+v"(wd[1]), "+v"(wd[2]), "+v"(wd[3]), "+v"(wd[4]), "+v"(wd[5]), "+v"(wd[6]), "+v"(wd[7]), "+v"(wd[8]), "+v"(bd), "+v"(gbias),
                   "+v"(gh[0]), "+v"(gh[1]), "+v"(gh[2]), "+v"(gh[3]), "+v"(gh[4]), "+v"(gh[5]), "+v"(gl[0]), "+v"(gl[1]), "+v"(gl[2]), "+v"(gl[3]), "+v"(gl[4]), "+v"(gl[5])
                 :: "memory");
    float amax = 0.0f;                                      // range guard (yn_split.h)
    const int j4 = lane & 3;
    const int nq = wave * 32 + (l31 & ~3);
    const unsigned wbase = (unsigned)ry * WROW + (unsigned)((rx * CQ + cq) * 16);     // the thread's top-left window granule
    // thread = (channel quad, run of four pixels along x): its 3 x 6 window row by row (18 sixteen-byte LDS reads), four independent fma chains in
    // dwconv3x3_kernel's order - bias, then ky, kx.  MASKED: zero padding and idle rows (nothing valid) as per-thread validity bits (`wok`),
    // applied where the values are consumed (the clamped fetches brought real pixels there)
    auto depthwise = [&](auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
        unsigned wok = 0;                                   // validity of the 18 window positions, bit ky * 6 + j: valid rows x valid columns are ranges
        if constexpr (MASKED) {
            int tt = t;                                     // (opaque: one register for the thread's place instead of three held across the tile)
            asm volatile("" : "+v"(tt));
            const int rn = tt / CQ, oy = cur.oy0 + (rn >> 1), ox = cur.ox0 + (rn & 1) * R;
            const int jlo = ox < 1 ? 1 - ox : 0, jhi = min(max(a.W + 1 - ox, 0), R + 2);        // columns [jlo, jhi) lie inside the image
            const int klo = oy < 1 ? 1 - oy : 0, khi = oy < a.H ? min(a.H + 1 - oy, 3) : 0;     // rows [klo, khi); an idle run has none
            const unsigned xb = jhi > jlo ? (1u << jhi) - (1u << jlo) : 0u, yb = khi > klo ? (1u << khi) - (1u << klo) : 0u;
            wok = ((yb & 1u) ? xb : 0u) | ((yb & 2u) ? xb << (R + 2) : 0u) | ((yb & 4u) ? xb << (2 * (R + 2)) : 0u);
        }
        const unsigned char* wp = win + wbase;
        float4 acc[R];
#pragma unroll
        for (int o = 0; o < R; ++o) acc[o] = make_float4(bd.x, bd.y, bd.z, bd.w);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            float4 row[R + 2];
#pragma unroll
            for (int j = 0; j < R + 2; ++j) {
                row[j] = *reinterpret_cast<const float4*>(wp + ky * WROW + j * (CQ * 16));
                if constexpr (MASKED) row[j] = vmask(row[j], 0u - ((wok >> (ky * (R + 2) + j)) & 1u));
            }
#pragma unroll
            for (int o = 0; o < R; ++o)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const f32x4 w = wd[ky * 3 + kx];
                    vfma(acc[o], row[o + kx], make_float4(w.x, w.y, w.z, w.w));
                }
        }
#pragma unroll
        for (int o = 0; o < R; ++o) {
            const float4 v = vact(acc[o], a.dw_act);
            const int op = ry * TW + rx + o;
            const float x4[4] = {v.x, v.y, v.z, v.w};
            h16x4 hi, lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) { amax = range_track(amax, x4[j]); hi[j] = (h16)x4[j]; lo[j] = split_lo(x4[j], hi[j]); }
            *reinterpret_cast<h16x4*>(Ah + op * AST + c) = hi;
            *reinterpret_cast<h16x4*>(Al + op * AST + c) = lo;
        }
    };
    lds_barrier();                                          // every wavefront's pieces of the first window

    for (;;) {
        // ---- 1. depthwise (dwconv3x3_kernel's chain) from the LDS window -> split planes.  A tile whose window lies inside the image (a
        //      wave-uniform test: most tiles of a large map) has nothing to zero and runs without the masks - the same values, the same bits ----
        if (cur.oy0 >= 1 && cur.oy0 + TH < a.H && cur.ox0 >= 1 && cur.ox0 + TW < a.W) depthwise(std::false_type{});
        else depthwise(std::true_type{});
        lds_barrier();                                      // planes complete; every window read has returned: the window buffer is free
        if (t1 >= 0) { nxt = decode(t1); issue(nxt); }      // the next tile's window flies under the GEMM and the epilogue's arithmetic

        // ---- 2. pointwise conv: 32 x 32 per wavefront, K = 96 in gemm_split_tile's order; bias, activation, 16-byte stores -------------
        f32x16 acc0, acc1;
#pragma unroll
        for (int k = 0; k < 16; ++k) { acc0[k] = 0.0f; acc1[k] = 0.0f; }
        const h16* Ahb = Ah + l31 * AST + h * 8;
        const h16* Alb = Al + l31 * AST + h * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h16x8 ah = *reinterpret_cast<const h16x8*>(Ahb + ks * 16);
            const h16x8 al = *reinterpret_cast<const h16x8*>(Alb + ks * 16);
            split_mfma(ah, al, gh[ks], gl[ks], acc0, acc1);
        }
        // tile pixel of accumulator group g, lane (h, j4): row g, column 4 h + j4 - a wave-uniform row offset + one lane offset, 32-bit
        char* obase = reinterpret_cast<char*>(a.out);
        const unsigned lane_off = (unsigned)(((cur.b * a.H + cur.oy0) * a.W + cur.ox0 + 4 * h + j4) * C + nq) * 4u;
        const bool xin = cur.ox0 + 4 * h + j4 < a.W;
        float4 ov[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v0 = apply_act(split_join(acc0[4 * g + 0], acc1[4 * g + 0]) + gbias, a.act);
            float v1 = apply_act(split_join(acc0[4 * g + 1], acc1[4 * g + 1]) + gbias, a.act);
            float v2 = apply_act(split_join(acc0[4 * g + 2], acc1[4 * g + 2]) + gbias, a.act);
            float v3 = apply_act(split_join(acc0[4 * g + 3], acc1[4 * g + 3]) + gbias, a.act);
            {   // 2x2 blocks, then 4x4: lane j of the quad ends up with row j x 4 columns (gemm_epilogue's transpose)
                const float s0 = (j4 & 1) ? v0 : v1, s1 = (j4 & 1) ? v2 : v3;
                const float r0 = quad_xor1(s0), r1 = quad_xor1(s1);
                if (j4 & 1) { v0 = r0; v2 = r1; } else { v1 = r0; v3 = r1; }
            }
            {
                const float s0 = (j4 & 2) ? v0 : v2, s1 = (j4 & 2) ? v1 : v3;
                const float r0 = quad_xor2(s0), r1 = quad_xor2(s1);
                if (j4 & 2) { v0 = r0; v1 = r1; } else { v2 = r0; v3 = r1; }
            }
            ov[g] = make_float4(v0, v1, v2, v3);
        }
        // this wavefront's pieces of the next window, in front of the stores (which share the counter and need not be waited for: what is in
        // flight here is the eight pieces and the previous tile's stores, issued a whole tile ago)
        if (t1 >= 0) vm_drain();
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (cur.oy0 + g < a.H && xin) *reinterpret_cast<float4*>(obase + (lane_off + (unsigned)(g * a.W * C) * 4u)) = ov[g];
        if (t1 < 0) break;
        cur = nxt;
        t1 = t1 + GL < tend ? t1 + GL : -1;
        lds_barrier();                                      // every wavefront is done with the planes, and has waited for its pieces of the next window
    }
    range_report(a.ovf, amax);
}

// three wavefronts per SIMD (168 registers): four workgroups of three wavefronts per CU
__global__ __attribute__((amdgpu_flat_work_group_size(192, 192), amdgpu_waves_per_eu(3, 3))) void dwpw_pipe_group_kernel(Group<DwPwArgs> g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dwpw_smem[];
    unsigned local, nb;
    const int p = group_problem(g.first, blockIdx.x, local, nb);
    dwpw_pipe_block(g.a[p], dwpw_smem, local, nb);
}

bool dwpw_group_ok(const DwPwArgs* a, int n)
{
    if (n < 1 || n > YN_GROUP_MAX) return false;
    for (int p = 0; p < n; ++p) {
        if (a[p].C != 96 || a[p].Npad != 96 || !a[p].Wh || !a[p].Wl || a[p].B <= 0) return false;
        if ((size_t)a[p].B * a[p].H * a[p].W * 96 >= ((size_t)1 << 30)) return false;      // 32-bit byte offsets
    }
    return true;
}

// Walking workgroups of every problem: ceil(tiles / 3) rounded up to a multiple of 8 (XCD-contiguous ranges: GL = grid / 8 tiles per step), or -
// where that is more than the chip holds at four workgroups per CU - the fewest steps S with which all levels fit the resident slots
// together, every level's workgroups walking at most S tiles (416 x 416, 32 images: 728 + 224 + 64 workgroups, 4 steps).
static void dwpw_group_grid(const DwPwArgs* a, int n, unsigned (&wgs)[YN_GROUP_MAX])
{
    constexpr unsigned per = 3;                             // at least this many tiles per walking workgroup
    unsigned TL[YN_GROUP_MAX] = {}, all = 0, tot = 0;       // TL: tiles per XCD range
    for (int p = 0; p < YN_GROUP_MAX; ++p) {
        wgs[p] = 0;
        if (p >= n) continue;
        const unsigned tiles = (unsigned)a[p].B * ((a[p].H + 3) / 4) * ((a[p].W + 7) / 8);
        TL[p] = (tiles + 7u) >> 3;
        wgs[p] = xcd_grid((tiles + per - 1) / per);
        all += tiles;
        tot += wgs[p];
    }
    if (tot <= DWPW_SLOTS) return;
    for (unsigned S = (all + DWPW_SLOTS - 1) / DWPW_SLOTS > per ? (all + DWPW_SLOTS - 1) / DWPW_SLOTS : per;; ++S) {
        unsigned used = 0;
        for (int p = 0; p < n; ++p) used += 8u * ((TL[p] + S - 1) / S);
        if (used > DWPW_SLOTS) continue;                    // (ends: 8 n workgroups at the latest)
        for (int p = 0; p < n; ++p) { const unsigned w = 8u * ((TL[p] + S - 1) / S); if (w < wgs[p]) wgs[p] = w; }
        return;
    }
}

void launch_dwpw_group(const DwPwArgs* a, int n, hipStream_t s)
{
    Group<DwPwArgs> g{};
    unsigned tot = 0, wgs[YN_GROUP_MAX];
    dwpw_group_grid(a, n, wgs);
    for (int p = 0; p < YN_GROUP_MAX; ++p) {
        g.first[p] = tot;
        if (p < n) { g.a[p] = a[p]; tot += wgs[p]; }
    }
    g.first[YN_GROUP_MAX] = tot;
    set_last_kernel_name("dwpw_pipe_group_kernel");
    hipLaunchKernelGGL(dwpw_pipe_group_kernel, dim3(tot), dim3(192), (size_t)DWPW_LDS, s, g);
}

bool launch_unit_chain(const ChainArgs& a, hipStream_t s) { return unit_chain_dispatch(a, s, false); }
bool unit_chain_covers(const ChainArgs& a) { return unit_chain_dispatch(a, nullptr, true); }

}  // namespace ynk
