// odpd_wide.h — what the one-sequence-per-wave, lane = hidden unit kernels have in common (gru_wide.hip, lstm_wide.hip, vdlstm_wide.hip,
// delta_wide.hip, deltajanet_wide.hip; from janet_wide.hip, gru_layers2.hip and lstm_layers2.hip, whose lanes mean something else, only the
// pieces that are literally the same code): the chunk constants, the W_hh row load, the broadcast mat-vec's float4 step, the start of the
// dW_hh accumulators and of the partial row, the wave sums, and the host side's grid, launch and dispatch.  A file uses a device helper
// only where its step loops keep their instruction sequence (docs/design/wide.md lists which); the cells, the record layouts, the chunk
// and step loops, the heads and the dL/dx collection stay in their files.
#pragma once
#include <type_traits>

#include "odpd_seq.h"

namespace odpd {

constexpr int kWC = 64;                               // time steps per chunk
constexpr int kWS = 65;                               // row stride of the per-chunk [time][unit] arrays (lane = unit and lane = time accesses both conflict-free)
constexpr int kWHs = ((kWC + 1) * kWS + 3) & ~3;      // floats of the [65][65] state array, padded so that what follows stays 16-byte aligned

// the W_hh rows of gates 0 .. NG-1 of this lane's unit, zero beyond H (row- and column-wise)
template <int NG>
__device__ __forceinline__ void wide_load_rows(float (&whh)[NG][64], const float* pl, int o_w_hh, int H, int lane, bool vo) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int k = 0; k < 64; ++k) whh[g][k] = (vo && k < H) ? pl[o_w_hh + (g * H + lane) * H + k] : 0.0f;
}

// one float4 of the broadcast state against columns 4 q .. 4 q + 3 of the lane's rows: acc[g] += whh[g][4 q ..] . hv
template <int NG, int NA>
__device__ __forceinline__ void wide_fma4(float (&acc)[NA], const float (&whh)[NG][64], int q, float4 hv) {
    static_assert(NG <= NA, "one accumulator per gate");
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        acc[g] = __builtin_fmaf(whh[g][4 * q], hv.x, acc[g]); acc[g] = __builtin_fmaf(whh[g][4 * q + 1], hv.y, acc[g]);
        acc[g] = __builtin_fmaf(whh[g][4 * q + 2], hv.z, acc[g]); acc[g] = __builtin_fmaf(whh[g][4 * q + 3], hv.w, acc[g]);
    }
}

// dW_hh accumulates as outer products on the 4-block MFMA: acc[g][rr], block b of rotation rr = units 16 b .. (rows) x units
// 16 ((b + rr) % 4) .. (columns).  The accumulation itself, the write-out of the accumulators and the column mat-vec over the gate
// gradients are spelled out in every file: moved into a helper, each changed the step loops' instruction sequence or a kernel's scratch
// bytes in nearly every file it was tried in (profiles/wide_refactor.md).
template <int NG>
__device__ __forceinline__ void wide_zero_acc(f32x16 (&acc)[NG][4]) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[g][r][i] = 0.0f;
}

// the workgroup's row of partial gradients, every entry zero before the lanes write their own (n = parameters + loss columns)
__device__ __forceinline__ float* wide_partial_row(float* partials, int n, int lane) {
    float* prow = partials + (size_t)blockIdx.x * n;
    for (int i = lane; i < n; i += 64) prow[i] = 0.0f;
    __builtin_amdgcn_s_waitcnt(0);
    wave_lds_fence();
    return prow;
}
// the per-time-lane accumulators, summed over the wave
template <int N>
__device__ __forceinline__ void wide_sum_lanes(float (&t)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = wave_sum64(t[i]);
}

// ---- host side ---------------------------------------------------------------------------------
// one single-wave workgroup per sequence until every CU has four; beyond, the workgroups loop over the batch
static inline int wide_rows(int B) { const int cap = 4 * device_cus(); return B < cap ? B : cap; }
template <typename K>
static inline int wide_launch(hipStream_t st, K kernel, size_t lds, const SeqArgs& a) {
    if (lds > kMaxLds) return ODPD_EUNSUPPORTED;      // (vdlstm's and the delta backbones' dL/dx grows with the frame)
    return launch_seq(st, kernel, wide_rows(a.B), lds, a);
}

}  // namespace odpd
