// yn_split.h — the split-f16 arithmetic of the inference kernels, written once: the f16 vector types, the range guard, the
// split x = hi + lo * 2^-11, the three MFMAs of a 16-deep k-step on split operands, the join of the two accumulators.  Included through
// yn_device.h; tests/test_capi_cpu.py keeps the MFMA builtin and the join's constant out of every other source (kernels_h16.hip, fp16
// training, splits one operand only: another scheme).  Each helper keeps the statement ORDER of the code it replaced - hipcc schedules from it.
#pragma once
#include "yn_h16.h"

namespace ynk {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int N> struct H16Vec { typedef _Float16 type __attribute__((ext_vector_type(N))); };

constexpr float SPLIT_SCALE = 2048.0f;                      // lo carries the 11 bits behind hi's
constexpr float SPLIT_INV = 1.0f / 2048.0f;
// ---- range guard of the split-f16 family ----------------------------------------------------------------------------------
// x = hi + lo * 2^-11 takes hi = (f16)x: finite only for |x| < 65520.  Beyond that hi = +-inf, lo = -+inf, the three-MFMA sum is
// NaN (and a ReLU epilogue turns that NaN into 0), where the reference's fp32 conv is finite.  Every kernel that splits
// activations keeps the running max |x| of what it splits (one v_max_f32 per element, next to the five VALU ops of the split itself)
// and raises the handle's flag once per wavefront at its end; yn_range_status() reports it and the host shim re-runs on the f32-MFMA
// family (yn_exact_f32).  Folded WEIGHTS are checked once, at yn_fold_bn (fold_pack_kernel).  Tiny values need no guard: below the f16
// normal range hi loses bits (or flushes to 0) but lo = (x - hi) * 2^11 still carries x exactly to 11 bits more, i.e. an absolute
// error <= 2^-25 * 2^-11 - far below the fp32 round-off of any accumulation that also holds O(1) terms.
#ifdef YN_EXP_NO_RANGE                                      // timing experiment only: the guard compiled out
__device__ __forceinline__ float range_track(float amax, float) { return amax; }
__device__ __forceinline__ void range_report(unsigned*, float) {}
#else
__device__ __forceinline__ float range_track(float amax, float x) { return __builtin_fmaxf(amax, __builtin_fabsf(x)); }
__device__ __forceinline__ void range_report(unsigned* ovf, float amax)
{
    if (ovf && amax >= 65504.0f) atomicOr(ovf, 1u);         // +inf included; a NaN input is NaN in the reference too
}
#endif
// ---- the split ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ h16 split_lo(float x, h16 hi) { return (h16)((x - (float)hi) * SPLIT_SCALE); }

// N adjacent values -> one vector store into each plane; per element: range_track, hi, lo.  Most vector sites keep this sequence written out
// over split_lo (as a call the stores' address arithmetic moves in front of the conversions and hipcc schedules the code around it
// differently).  A value that is the result of an fma is first pinned as an fp32 register (asm volatile("" : "+v"(x)), the depthwise
// phases): else fma and conversion fold into v_fma_mixlo_f16 - one rounding - and 1 pixel of 200 gets another hi.
template <int N>
__device__ __forceinline__ void split_store(h16* hi_dst, h16* lo_dst, float (&v)[N], float& amax)
{
    typename H16Vec<N>::type hi, lo;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        amax = range_track(amax, v[j]);
        hi[j] = (h16)v[j];
        lo[j] = split_lo(v[j], hi[j]);
    }
    *reinterpret_cast<typename H16Vec<N>::type*>(hi_dst) = hi;
    *reinterpret_cast<typename H16Vec<N>::type*>(lo_dst) = lo;
}

// ---- one 16-deep k-step on split operands: hi*hi into acc0, the two cross terms into acc1 (lo*lo is below fp32's round-off) ----
__device__ __forceinline__ void split_mfma(const h16x8 ah, const h16x8 al, const h16x8 bh, const h16x8 bl, f32x16& acc0, f32x16& acc1)
{
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc1, 0, 0, 0);
}

// (B fragments of a resident register panel go by address: by value down_unit_pipe_kernel's GEMMs are scheduled differently)
__device__ __forceinline__ void split_mfma(const h16x8 ah, const h16x8 al, const h16x8* bh, const h16x8* bl, f32x16& acc0, f32x16& acc1)
{
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, *bh, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, *bl, acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, *bh, acc1, 0, 0, 0);
}

// ---- the join: acc0 + acc1 * 2^-11, one fma per element ----
__device__ __forceinline__ float split_join(float acc0, float acc1) { return __builtin_fmaf(acc1, SPLIT_INV, acc0); }
__device__ __forceinline__ void split_join(f32x16& acc0, const f32x16& acc1)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = split_join(acc0[r], acc1[r]);
}

}  // namespace ynk
