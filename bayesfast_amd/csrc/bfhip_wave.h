// bfhip_wave.h -- wave-level helpers of the wave-per-chain sampler kernels (gfx950): DPP moves, uniform-value hints, the
// 64-lane sums on the idle matrix pipe.  Included by bfhip_sampler.hip and bfhip_tnuts.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one DPP move of a double (both halves)
template <int CTRL>
__device__ inline double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ inline double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Wave-uniform values that arrive through a vector load (LDS, global memory) or an out-of-line call look
// divergent to the compiler, which then keeps the whole chain state machine in VGPRs and lowers its branches to
// exec-mask manipulation.  rfl() states the uniformity: the value moves to scalar registers and everything
// derived from it (unit, mode, depth, the branch conditions) stays scalar.
__device__ inline int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline double rfl(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ inline uint64_t rfl(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// gfx950 row swaps: every lane ends with (its row) + (the neighbouring row), then (its half) + (the other half)
__device__ inline double swap16_add_f64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
__device__ inline double swap32_add_f64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
// Sums over the 64 lanes of N independent values, wave-uniform results in a fixed order.  The N reductions advance
// step by step together so that the latency of each step is covered by the other values' instructions.
// Default (wave_sum_n_packed): one v_mfma_f64_4x4x4 per value, then one more and two row rotations per FOUR values (the
// FP64 vector instructions share the SIMD's pipe with the MFMAs, and the pipelined kernel's trip is bound by that pipe:
// docs/EXPERIMENTS.md); with BF_WSUM_UNPACKED (wave_sum_n_unpacked): the second MFMA and the rotations once per value,
// the same numbers; with BF_WSUM_BUTTERFLY: four DPP butterfly steps inside the rows of 16 lanes and two gfx950 row swaps
// (11 % slower on the headline workload, kept as the reference form of the reduction).
//
// v_mfma_f64_4x4x4 is four 4 x 4 x 4 products, one per block b = (lane >> 2) & 3: A[i][k] comes from lane 16k + 4b + i,
// B[k][j] from lane 16k + 4b + j, D[i][j] = sum_k A[i][k] B[k][j] (k ascending) lands in lane 16i + 4b + j.
// With B = 1 the first MFMA leaves, in lane 16i + 4b + j, the sum of the four lanes 16k + 4b + i (k = 0..3); fed back as the
// B operand with A = 1 the second sums those over i: every lane of block b holds the total of its block's 16 lanes; two row
// rotations add the four blocks.
template <int N>
__device__ inline void wave_sum_n_unpacked(double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(v[i], 1., 0., 0, 0, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(1., v[i], 0., 0, 0, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0x128>(v[i]);  // row_ror:8
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0x124>(v[i]);  // row_ror:4
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = rfl(v[i]);
}
// The reduction with its results left where the arithmetic puts them (default form: the packs after the two row rotations, every
// lane of column j of pack c holding value 4 c + j; a padding column of a short pack repeats one of the pack's own values).
// get(i) reads one value into scalar registers -- the bits of wave_sum_n --, any_le0() asks whether some value is <= 0. (ordered:
// false for NaN, true for +-0. and -inf) with one compare per pack on the packed register, the lane masks OR-ed on the scalar
// unit: a U-turn test, which wants nothing but that answer, reads no sum.  With BF_WSUM_UNPACKED / BF_WSUM_BUTTERFLY the values
// are wave-uniform already and the test is the scalar expression; BF_UTURN_READ_ALL keeps that read-everything form of the test
// in the default build too (tools/svariant.sh readall -DBF_UTURN_READ_ALL, for a comparison on the device).
#if defined(BF_WSUM_UNPACKED) || defined(BF_WSUM_BUTTERFLY)
#define BF_WSUM_UNIFORM 1
#endif
template <int N>
struct WavePacks {
#ifdef BF_WSUM_UNIFORM
    static constexpr int NP = N;
#else
    static constexpr int NP = N == 1 ? 1 : (N + 3) / 4;
#endif
    double pk[NP];
    __device__ inline double get(int i) const {
#ifdef BF_WSUM_UNIFORM
        return pk[i];
#else
        if constexpr (N == 1) return rfl(pk[0]);
        else return (i & 3) ? readlane_f64(pk[i >> 2], i & 3) : rfl(pk[i >> 2]);
#endif
    }
    __device__ inline bool any_le0() const {
#if defined(BF_WSUM_UNIFORM) || defined(BF_UTURN_READ_ALL)
        bool t = false;
#pragma unroll
        for (int i = 0; i < N; ++i) t = t || (get(i) <= 0.);
        return t;
#else
        uint64_t mask = 0;
#pragma unroll
        for (int c = 0; c < NP; ++c) mask |= __builtin_amdgcn_ballot_w64(pk[c] <= 0.);
        return mask != 0;
#endif
    }
};
// The first MFMA's result is the same in the four columns j of a block, and the second MFMA and the rotations (by 8 and 4
// lanes) never mix columns: the unpacked form does the same arithmetic four times over.  Here column j carries value
// 4 c + j of pack c -- the operand of the second step takes lane l from value (l & 3) -- and value 4 c + j is read from
// lane j.  Every column sees the operations of the unpacked form in the same order: bit-identical results, and a NaN or
// an infinity stays in its own value's column.  (Like the rotations of the unpacked form, this wants all 64 lanes active:
// the callers reduce under wave-uniform control flow only.)
// (the packed form by name -- the probe runs it whatever the library was built with --: the packs after the two row rotations)
template <int N>
__device__ inline void wave_packs_packed(double (&v)[N], double (&pk)[N == 1 ? 1 : (N + 3) / 4]) {
    if constexpr (N == 1) {
        // (one value: nothing to pack; the unpacked form without its read)
        double t = __builtin_amdgcn_mfma_f64_4x4x4f64(v[0], 1., 0., 0, 0, 0);
        t = __builtin_amdgcn_mfma_f64_4x4x4f64(1., t, 0., 0, 0, 0);
        t += dpp_f64<0x128>(t);  // row_ror:8
        t += dpp_f64<0x124>(t);  // row_ror:4
        pk[0] = t;
    } else {
        constexpr int NP = (N + 3) / 4;
        const bool odd = threadIdx.x & 1, upper = threadIdx.x & 2;   // bits 0 and 1 of the lane
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(v[i], 1., 0., 0, 0, 0);
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const int b = 4 * c, m = (N - b < 4) ? N - b : 4;   // the values of this pack; a column without one repeats another
            const int i1 = m >= 2 ? b + 1 : b, i2 = m >= 3 ? b + 2 : b, i3 = m >= 4 ? b + 3 : i2;
            // (selects between values, not between the array's elements: those would keep the array in scratch memory)
            const double a0 = v[b], a1 = v[i1], a2 = v[i2], a3 = v[i3];
            const double lo = odd ? a1 : a0, hi = odd ? a3 : a2;
            pk[c] = (m >= 3) ? (upper ? hi : lo) : lo;
        }
#pragma unroll
        for (int c = 0; c < NP; ++c) pk[c] = __builtin_amdgcn_mfma_f64_4x4x4f64(1., pk[c], 0., 0, 0, 0);
#pragma unroll
        for (int c = 0; c < NP; ++c) pk[c] += dpp_f64<0x128>(pk[c]);  // row_ror:8
#pragma unroll
        for (int c = 0; c < NP; ++c) pk[c] += dpp_f64<0x124>(pk[c]);  // row_ror:4
    }
}
template <int N>
__device__ inline void wave_sum_n_packed(double (&v)[N]) {
    double pk[N == 1 ? 1 : (N + 3) / 4];
    wave_packs_packed<N>(v, pk);
    if constexpr (N == 1) {
        v[0] = rfl(pk[0]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = (i & 3) ? readlane_f64(pk[i >> 2], i & 3) : rfl(pk[i >> 2]);
    }
}
template <int N>
__device__ inline void wave_sum_n_butterfly(double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0xB1>(v[i]);   // quad_perm [1,0,3,2]
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0x4E>(v[i]);   // quad_perm [2,3,0,1]
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0x141>(v[i]);  // row_half_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f64<0x140>(v[i]);  // row_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = swap16_add_f64(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = swap32_add_f64(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = rfl(v[i]);
}
// (v is used up: it holds intermediate values afterwards)
template <int N>
__device__ inline WavePacks<N> wave_sum_packs(double (&v)[N]) {
    WavePacks<N> r;
#if defined(BF_WSUM_UNPACKED)
    wave_sum_n_unpacked<N>(v);
#pragma unroll
    for (int i = 0; i < N; ++i) r.pk[i] = v[i];
#elif defined(BF_WSUM_BUTTERFLY)
    wave_sum_n_butterfly<N>(v);
#pragma unroll
    for (int i = 0; i < N; ++i) r.pk[i] = v[i];
#else
    wave_packs_packed<N>(v, r.pk);
#endif
    return r;
}
template <int N>
__device__ inline void wave_sum_n(double (&v)[N]) {
    const WavePacks<N> r = wave_sum_packs<N>(v);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = r.get(i);
}
__device__ inline double wave_sum(double v) {
    double t[1] = {v};
    wave_sum_n<1>(t);
    return t[0];
}

