// odpd_qcell.h — what the in-cell quantised kernels (`--quant` on a backbone whose nn.Linear all become INT_Linear: pgjanet_q.hip, bojanet_q.hip,
// dvrjanet_q.hip) have in common: the parameter layout of a chain of INT_Linear, the staging of the parameters in LDS with the weight matrices
// quantised in place, the write-out of a workgroup's row of weight-gradient partials, and the two register-row primitives of a single-wave
// recurrence.  A backbone's file keeps what is its own: its front, its recurrence and its head (docs/design/quantised.md, "The shared header").
// Nothing here is contraction-sensitive: every multiply-add is an explicit __builtin_fmaf.
#pragma once
#include "odpd_seq.h"
#include "odpd_quant.h"

namespace odpd {
namespace qcell {

// ---- parameter layout ---------------------------------------------------------------------------
// The quantised model's named_parameters(): per INT_Linear its weight at ow[l], its bias at ob[l] (= oq[l] where the layer has none) and its
// three scale parameters at oq[l] — weight scale, activation scale, output scale (quant/qmodules/quant_layers.py:48-85).  P: the total.
template <int NL> struct QcLayout { int ow[NL], ob[NL], oq[NL], P; };
struct QcLinear { int nout, nin; bool bias; };
// fills L for the layers shape(0) .. shape(NL - 1) (each a QcLinear), the first of them at offset `first`
template <int NL, typename Shape>
__host__ __device__ inline void qc_fill_layout(QcLayout<NL>& L, int first, Shape shape) {
    int o = first;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const QcLinear s = shape(l);
        L.ow[l] = o; o += s.nout * s.nin;
        L.ob[l] = o; if (s.bias) o += s.nout;
        L.oq[l] = o; o += 3;
    }
    L.P = o;
}
inline bool qc_bits_ok(const odpd_model_t* m) { return m->bits_w > 0 && m->bits_w <= 16 && m->bits_a > 0 && m->bits_a <= 16; }

// ---- setup --------------------------------------------------------------------------------------
__device__ __forceinline__ void qc_uniform(q16::Quant& q) { q.s = uni_(q.s); q.inv = uni_(q.inv); }
// stage the parameters in pl, form every layer's activation quantiser (qa), quantise the NL weight matrices in the staged copy.
// UNI: the activation quantisers' scales go through qc_uniform as they are formed.  That is a choice of the kernel, not of the layout: bojanet_q
// and dvrjanet_q apply them on lanes of every role and want them in scalar registers; pgjanet_q has never done so.  The step sits here, not
// behind the call, because the register allocation of the whole kernel follows its place (after the last fence: 6 to 8 VGPRs fewer in
// every bjq_ / dvq_ kernel — another occupancy for two of them, and not the kernels that were measured).
template <bool UNI, int NL>
__device__ __forceinline__ void qc_setup(float* pl, const SeqArgs& a, const QcLayout<NL>& L, q16::Quant (&qa)[NL], int lane) {
    stage_params(pl, a.params, L.P);
    wave_lds_fence();
    q16::Quant qw[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        qa[l] = q16::make_quant(pl[L.oq[l] + 1], a.bits_a);
        if constexpr (UNI) qc_uniform(qa[l]);
        qw[l] = q16::make_quant(pl[L.oq[l]], a.bits_w);
    }
    wave_lds_fence();
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int n = L.ob[l] - L.ow[l];
        for (int i = lane; i < n; i += 64) pl[L.ow[l] + i] = q16::qapply(pl[L.ow[l] + i], qw[l]);
    }
    wave_lds_fence();
}

// ---- write-out ----------------------------------------------------------------------------------
// the workgroup's row of partials from gw (the weight gradients in the parameter layout, in LDS): the weight quantisers' pass masks from the
// unquantised weights, the scale columns exact zeros (round() inside the quantiser: quantizers.py:56-65), the loss columns zero
template <int NL>
__device__ __forceinline__ void qc_write_partials(const SeqArgs& a, const QcLayout<NL>& L, const float* gw, int lane) {
    float* prow = a.partials + (size_t)blockIdx.x * (L.P + kLossCols);
    q16::Quant qw[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) qw[l] = q16::make_quant(a.params[L.oq[l]], a.bits_w);
    for (int i = lane; i < L.P + kLossCols; i += 64) {
        float v = i < L.P ? gw[i] : 0.0f;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (i >= L.ow[l] && i < L.ob[l]) v *= q16::qpass(a.params[i], qw[l]);
            if (i >= L.oq[l] && i < L.oq[l] + 3) v = 0.0f;
        }
        prow[i] = v;
    }
}

// ---- a row in registers against a vector in LDS --------------------------------------------------
// acc + sum_k w[k] v[k], k ascending, one FMA chain; v is read as N / 4 float4 (every lane the same address: broadcasts)
template <int N>
__device__ __forceinline__ float qc_dot(const float (&w)[N], const float* v, float acc) {
    static_assert(N % 4 == 0, "the vector is read as float4");
#pragma unroll
    for (int q4 = 0; q4 < N / 4; ++q4) {
        const float4 x = *reinterpret_cast<const float4*>(v + 4 * q4);
        acc = __builtin_fmaf(w[4 * q4], x.x, acc); acc = __builtin_fmaf(w[4 * q4 + 1], x.y, acc);
        acc = __builtin_fmaf(w[4 * q4 + 2], x.z, acc); acc = __builtin_fmaf(w[4 * q4 + 3], x.w, acc);
    }
    return acc;
}
// the matching rank-1 update of a gradient row: g[k] += d v[k]
template <int N>
__device__ __forceinline__ void qc_axpy(float (&g)[N], float d, const float* v) {
    static_assert(N % 4 == 0, "the vector is read as float4");
#pragma unroll
    for (int q4 = 0; q4 < N / 4; ++q4) {
        const float4 x = *reinterpret_cast<const float4*>(v + 4 * q4);
        g[4 * q4] = __builtin_fmaf(d, x.x, g[4 * q4]); g[4 * q4 + 1] = __builtin_fmaf(d, x.y, g[4 * q4 + 1]);
        g[4 * q4 + 2] = __builtin_fmaf(d, x.z, g[4 * q4 + 2]); g[4 * q4 + 3] = __builtin_fmaf(d, x.w, g[4 * q4 + 3]);
    }
}

}  // namespace qcell
}  // namespace odpd
