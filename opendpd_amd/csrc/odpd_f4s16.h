// odpd_f4s16.h — what the float 16-sequences-per-wave kernels of pgjanet, bojanet, apnrru, dvrjanet and mcldnn have in common (janet_s16.hip,
// bojanet_s16.hip, apnrru_s16.hip, dvrjanet_s16.hip, mcldnn.hip): the weight-table build, the frame chunk with a halo of bojanet's and
// apnrru's FIR banks, the backward epilogue's sum over the waves, and the host side's launch shape (the backward's dispatch,
// s16_bwd_dispatch, is in odpd_host.h).  The cells, the block functions and the kernels' own loops stay in their files
// (docs/design/f4_backbones.md).
#pragma once
#include "odpd_s16.h"

namespace odpd {

// the weight table [group][lane] float4: ENTRY is the file's own *_entry(extra..., pl, L, grp, m = lane & 15, q = lane >> 4), the groups dealt
// to the waves.  (The entry function is a template argument and `pl` a value: handed over as a lambda that captures them, the same loop
// moved the register allocation of dvr16_bwd_kernel, boj16_bwd_kernel and apn16_bwd_kernel.)
template <int NG, auto ENTRY, typename Layout, typename... Extra>
__device__ __forceinline__ void s16_build_table(float* tab, const float* pl, const Layout& L, int lane, int wave, int nwb, const Extra&... extra) {
    float4* t4 = reinterpret_cast<float4*>(tab);
    for (int grp = wave; grp < NG; grp += nwb) t4[grp * 64 + lane] = ENTRY(extra..., pl, L, grp, lane & 15, lane >> 4);
    __syncthreads();
}

// ---- frame chunk with a halo: 16 sequences x (HALO + kChunk) samples, index i <-> time t0 - HALO + i, float2 row stride kHaloRow ----
constexpr int kHalo = 16;                           // staged samples before the chunk (15 used: the 16 taps reach back to t - 15)
constexpr int kHaloRow = kHalo + kChunk + 1;
// Before the frame: zeros (the reference pads its frame on the left: bojanet.py:72-73, apnrru.py:68-69).  Idle sequence slots: any finite,
// non-degenerate signal.  Steps past t0 + len are computed and dropped: bojanet (IDLE_TAIL false) zero-fills them — its demodulator takes a
// filter output of 0 —, apnrru (IDLE_TAIL true) divides by |x_t| and needs a finite signal with |x| > 0 there as well.
template <int HALO, bool IDLE_TAIL>
__device__ __forceinline__ void halo_stage_in(float2* lds, const float* g, int b0, int B, int T, int t0, int len, int lane) {
    static_assert(HALO + kChunk + 1 == kHaloRow, "one row stride for every halo kernel");
    const float2* g2 = reinterpret_cast<const float2*>(g);
    constexpr int W = HALO + kChunk;
#pragma unroll
    for (int j = 0; j < 16 * W / 64; ++j) {
        const int e = lane + 64 * j, m = e / W, i = e % W, t = t0 - HALO + i;
        float2 v = make_float2(0.0f, 0.0f);
        if (b0 + m >= B || (IDLE_TAIL && t >= t0 + len)) v = make_float2(0.5f, 0.25f);
        else if (t >= 0 && (IDLE_TAIL || t < t0 + len)) v = g2[(size_t)(b0 + m) * T + t];
        lds[m * kHaloRow + i] = v;
    }
}
template <int HALO>
__device__ __forceinline__ void halo_stage_out(const float2* lds, float* g, int b0, int B, int T, int t0, int len, int lane) {
    float2* g2 = reinterpret_cast<float2*>(g);
#pragma unroll
    for (int j = 0; j < 16 * kChunk / 64; ++j) {
        const int e = lane + 64 * j, m = e / kChunk, tt = e % kChunk;
        if (tt < len && b0 + m < B) g2[(size_t)(b0 + m) * T + t0 + tt] = lds[m * kHaloRow + HALO + tt];
    }
}
// dL/dx chunk hand-over (backward runs the chunks last to first): what the finished chunk put before its own t0 (indices 1..HALO-1)
// belongs to the end of the next (earlier) one (indices kChunk+1..kChunk+HALO-1); everything else restarts at 0
template <int HALO>
__device__ __forceinline__ void halo_dx_carry(float2* lds, int lane, bool first) {
    constexpr int N = 16 * HALO / 64;
    float2 c[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = lane + 64 * j, m = e / HALO, i = e % HALO;
        c[j] = first ? make_float2(0.0f, 0.0f) : lds[m * kHaloRow + i];
    }
    wave_lds_fence();
    for (int e = lane; e < 16 * kHaloRow; e += 64) lds[e] = make_float2(0.0f, 0.0f);
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = lane + 64 * j, m = e / HALO, i = e % HALO;
        if (i) lds[m * kHaloRow + kChunk + i] = c[j];
    }
    wave_lds_fence();
}

// backward epilogue: every wave has deposited its row of P4 floats at smem + wave * P4 (and the workgroup has met at a barrier);
// the workgroup's row of partials is their sum
__device__ __forceinline__ void s16_reduce_rows(const float* smem, float* prow, int P4, int nwb) {
    for (int i = threadIdx.x; i < P4; i += blockDim.x) {
        float v = smem[i];
        for (int wv = 1; wv < nwb; ++wv) v += smem[wv * P4 + i];
        prow[i] = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------
// forward: four-wave workgroups until every CU has four of them, eight-wave ones beyond
static inline LaunchShape s16_fwd_shape(int ngroups) { return s16_group_shape(ngroups, ngroups <= 4 * device_cus() ? 4 : 8); }
}  // namespace odpd
