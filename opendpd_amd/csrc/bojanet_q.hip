// bojanet_q.hip — `--quant` on bojanet (reference quant/quant_envs.py:40-60, 145-148, 276-306 on backbones/bojanet.py:5-138): all eight nn.Linear of
// the backbone — fir_I, fir_Q (16 -> 6, no bias), W_fi, W_gi (12 -> H, bias), W_fh, W_gh (H -> H, no bias), W_out_I, W_out_Q (H -> 1, bias) — become
// INT_Linear (quant/qmodules/quant_layers.py:48-85): each quantises ITS input on an activation grid of its own and its weight on a weight grid
// (three scale parameters behind each layer's weight / bias); sigmoid, tanh, sqrt and the divisions are functional and stay float; no module is
// named fc_out, so the 16-bit output quantiser never runs (train mode = eval mode).  Selected by ODPD_FLAG_QUANT_CELL with bits_w, bits_a > 0.
//
// ONE sequence per single-wave workgroup (the form of boj_gp_eval_kernel / pgjanet_q.hip), in chunks of 64 steps.  Parameter layout, setup (the
// parameters staged in LDS with the eight weight matrices quantised IN PLACE) and write-out: odpd_qcell.h.  Per chunk:
//   front       lane = time step: the frame chunk is staged with a 16-sample halo as FOUR quantised copies (fir_I and fir_Q are each called on the
//               I window and on the Q window, bojanet.py:82-85: q_firI(I), q_firQ(I), q_firI(Q), q_firQ(Q)); the four 16-tap sums per filter,
//               fi = fir_I(I) - fir_Q(Q), fq = fir_Q(I) + fir_I(Q); the demodulator; the envelopes on W_fi's and on W_gi's activation grid; the
//               input halves W_fi q(e) + b, W_gi q(e) + b of both gates;
//   recurrence  lane = unit (rows f | g | f | g of the wave, the row's recurrent block in registers): q_fh(h), q_gh(h) broadcast through LDS, one
//               dot product per row, one cross-row swap, h' on every row;
//   head        lane = time step: phase re-rotation, q_outI(h cos), q_outQ(h sin), both read-outs (each feeds both outputs, :103-104).
// Every mat-vec sums k ascending (W8A8: products of grid values are integers below 2^14, sums of <= 16 of them exact in any order; W16A16 is not).
// Backward: the chunks last to first from a checkpoint of h per chunk — front and recurrence again (f, g, h of the chunk parked in LDS), the head's
// gradients with lane = time step, the reverse recurrence with lane = unit (transposed blocks in registers, every layer's activation pass mask;
// the weight gradients of W_fh, W_gh, W_fi, W_gi accumulate in the registers of the lane that owns the row), the demodulator's gradient with
// lane = time step, dL/dx as a gather over the 16 steps that see a sample (the first 15 steps of the later chunk are kept as a halo; each sample
// passes the masks of BOTH banks' activation quantisers), the FIR weight gradients with lane = (filter, tap).
// Deviation: where a filter output is exactly 0 + 0j — no measure-zero event with inputs on a grid — the reference's gradient is NaN (0 * inf
// through sqrt); here that term is dropped, as in bojanet_s16.hip.
#include "odpd_qcell.h"

#pragma clang fp contract(off)

namespace odpd {
namespace {
using namespace qcell;
constexpr int kQP = 6, kQM = 16, kQE = 2 * kQP;     // filters, taps, envelopes
constexpr int kQC = 64;                             // steps per chunk
constexpr int kQX = kQC + 16;                       // staged samples: index i <-> time t0 - 16 + i; also the row of dL/dfi, dL/dfq (64 .. 78: the later chunk's first steps)
constexpr int kQP16 = 17, kQP32 = 33;               // row pitches of the [time][unit] buffers: conflict-free for lane = unit and for lane = time
constexpr int kQL = 8;                              // 0 fir_I  1 fir_Q  2 W_fi  3 W_fh  4 W_gi  5 W_gh  6 W_out_I  7 W_out_Q (named_parameters order)
struct BjqLayout : QcLayout<kQL> { int H; };
__host__ __device__ inline int bjq_nin(int l, int H) { return l < 2 ? kQM : (l == 2 || l == 4) ? kQE : H; }
__host__ __device__ inline int bjq_nout(int l, int H) { return l < 2 ? kQP : l < 6 ? H : 1; }
__host__ __device__ inline BjqLayout bjq_layout(int H) {
    BjqLayout L; L.H = H;
    qc_fill_layout(L, 0, [H](int l) { return QcLinear{bjq_nout(l, H), bjq_nin(l, H), l == 2 || l == 4 || l >= 6}; });
    return L;
}
constexpr int kQHist = ((kQC + 1) * kQP16 + 3) & ~3;
__host__ __device__ inline int bjq_fwd_floats(int P) { return pad4(P) + 4 * kQX + kQE * kQC + kQP32 * kQC + kQHist + 32; }
__host__ __device__ inline int bjq_bwd_floats(int P) {
    return 2 * pad4(P) + 4 * kQX + kQE * kQC + 2 * kQC * kQE + 2 * kQP32 * kQC + kQHist + kQP16 * kQC + kQE * kQC + kQE * kQX + 2 * kQC + 64;
}

struct BjqQ { q16::Quant a[kQL]; };      // the layers' activation quantisers (wave-uniform)
// the chunk's samples with their halo, zero outside the frame (bojanet.py:72-73), on the four grids they are read on
__device__ __forceinline__ void bjq_stage_x(float4* xq, const float2* xg, int t0, int T, const BjqQ& Q, int lane) {
    for (int i = lane; i < kQX; i += 64) {
        const int t = t0 - 16 + i;
        float2 v = make_float2(0.0f, 0.0f);
        if (t >= 0 && t < T) v = xg[t];
        xq[i] = make_float4(q16::qapply(v.x, Q.a[0]), q16::qapply(v.x, Q.a[1]), q16::qapply(v.y, Q.a[0]), q16::qapply(v.y, Q.a[1]));
    }
}
struct BjqDemod { float m0, mag, co, si; };
__device__ __forceinline__ BjqDemod bjq_demod(float fi, float fq) {
    BjqDemod d;
    d.m0 = sqrtf(fi * fi + fq * fq); d.mag = d.m0 + 1e-8f;
    d.co = fi / d.mag; d.si = fq / d.mag;
    return d;
}
// front of local step tt (lane = time step): fi, fq -> fiq; input halves of both gates -> xs; QE: the envelopes on both gates' grids -> qe
template <bool QE>
__device__ __forceinline__ void bjq_front(const float* pl, const BjqLayout& L, const BjqQ& Q, const float4* xq, float* fiq, float* xs, float* qe, int tt) {
    float sII[kQP], sQI[kQP], sIQ[kQP], sQQ[kQP];
#pragma unroll
    for (int p = 0; p < kQP; ++p) { sII[p] = 0.0f; sQI[p] = 0.0f; sIQ[p] = 0.0f; sQQ[p] = 0.0f; }
#pragma unroll
    for (int m = 0; m < kQM; ++m) {
        const float4 v = xq[tt + 1 + m];                              // time t - 15 + m
#pragma unroll
        for (int p = 0; p < kQP; ++p) {
            const float wI = pl[L.ow[0] + p * kQM + m], wQ = pl[L.ow[1] + p * kQM + m];
            sII[p] = __builtin_fmaf(wI, v.x, sII[p]); sQI[p] = __builtin_fmaf(wQ, v.y, sQI[p]);
            sIQ[p] = __builtin_fmaf(wI, v.z, sIQ[p]); sQQ[p] = __builtin_fmaf(wQ, v.w, sQQ[p]);
        }
    }
    float ef[kQE], eg[kQE];
#pragma unroll
    for (int p = 0; p < kQP; ++p) {
        const float fi = sII[p] - sQQ[p], fq = sQI[p] + sIQ[p];
        fiq[p * kQC + tt] = fi; fiq[(kQP + p) * kQC + tt] = fq;
        const BjqDemod D = bjq_demod(fi, fq);
        const float mag2 = D.mag * D.mag;
        ef[p] = q16::qapply(D.mag, Q.a[2]); ef[kQP + p] = q16::qapply(mag2, Q.a[2]);
        eg[p] = q16::qapply(D.mag, Q.a[4]); eg[kQP + p] = q16::qapply(mag2, Q.a[4]);
    }
    if constexpr (QE) {
#pragma unroll
        for (int k = 0; k < kQE; ++k) { qe[tt * kQE + k] = ef[k]; qe[(kQC + tt) * kQE + k] = eg[k]; }
    }
#pragma unroll 1
    for (int u = 0; u < 16; ++u) {
        float pf = 0.0f, pg = 0.0f;
        if (u < L.H) {
#pragma unroll
            for (int k = 0; k < kQE; ++k) {
                pf = __builtin_fmaf(pl[L.ow[2] + u * kQE + k], ef[k], pf);
                pg = __builtin_fmaf(pl[L.ow[4] + u * kQE + k], eg[k], pg);
            }
            pf += pl[L.ob[2] + u]; pg += pl[L.ob[4] + u];
        }
        xs[tt * kQP32 + u] = pf; xs[tt * kQP32 + 16 + u] = pg;
    }
}
// the recurrence over the chunk's steps (lane = unit col of row f | g | f | g): entry tt + 1 of hist = h(t0 + tt); FG: f, g of the step parked
template <bool FG>
__device__ __forceinline__ float bjq_recur(const BjqQ& Q, const float (&w)[16], const float* xs, float* hist, float* fg, float* vq, int len, int lane,
                                           bool valid, float h) {
    const int col = lane & 15, role = lane >> 4;
    const bool is_f = (role & 1) == 0;
    const float* vr = vq + (is_f ? 0 : 16);
    const int xo = (is_f ? 0 : 16) + col;
    if (role == 0) hist[col] = h;
    for (int tt = 0; tt < len; ++tt) {
        if (role == 0) { vq[col] = q16::qapply(h, Q.a[3]); vq[16 + col] = q16::qapply(h, Q.a[5]); }
        wave_lds_fence();
        const float pre = xs[tt * kQP32 + xo] + qc_dot(w, vr, 0.0f);
        const float v = is_f ? sigmoidf_(pre) : tanhf_(pre), o = xor16(v);
        const float f = is_f ? v : o, g = is_f ? o : v;
        h = valid ? f * h + (1.0f - f) * g : 0.0f;
        if (role == 0) {
            hist[(tt + 1) * kQP16 + col] = h;
            if constexpr (FG) { fg[tt * kQP32 + col] = f; fg[tt * kQP32 + 16 + col] = g; }
        }
        wave_lds_fence();
    }
    return h;
}

template <bool SAVE>
__global__ __launch_bounds__(64) void bjq_fwd_kernel(SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, col = lane & 15, role = lane >> 4;
    const BjqLayout L = bjq_layout(a.H);
    const int H = L.H, T = a.T, NC = (T + kQC - 1) / kQC;
    float* pl = smem;
    float4* xq = reinterpret_cast<float4*>(smem + pad4(L.P));       // [80] q_firI(I), q_firQ(I), q_firI(Q), q_firQ(Q)
    float* fiq = reinterpret_cast<float*>(xq + kQX);                 // [12][64] fi_p, fq_p
    float* xs = fiq + kQE * kQC;                                     // [64][33] input halves of f | g
    float* hist = xs + kQP32 * kQC;                                  // [65][17]
    float* vq = hist + kQHist;                                       // [2][16] q_fh(h), q_gh(h)
    BjqQ Q;
    qc_setup<true>(pl, a, L, Q.a, lane);
    const bool valid = col < H;
    float w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = (valid && k < H) ? pl[((role & 1) ? L.ow[5] : L.ow[3]) + col * H + k] : 0.0f;
    if (lane < 32) vq[lane] = 0.0f;
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        float2* yg = reinterpret_cast<float2*>(a.y) + (size_t)b * T;
        float h = 0.0f;
        for (int c = 0; c < NC; ++c) {
            const int t0 = c * kQC, len = min(kQC, T - t0);
            if constexpr (SAVE) { if (role == 0) a.ckpt[((size_t)b * NC + c) * 16 + col] = h; }
            wave_lds_fence();
            bjq_stage_x(xq, xg, t0, T, Q, lane);
            wave_lds_fence();
            bjq_front<false>(pl, L, Q, xq, fiq, xs, nullptr, lane);
            wave_lds_fence();
            h = bjq_recur<false>(Q, w, xs, hist, nullptr, vq, len, lane, valid, h);
            if (lane < len) {      // the chunk's outputs, lane = time step
                float co[kQP], si[kQP];
#pragma unroll
                for (int p = 0; p < kQP; ++p) {
                    const BjqDemod D = bjq_demod(fiq[p * kQC + lane], fiq[(kQP + p) * kQC + lane]);
                    co[p] = D.co; si[p] = D.si;
                }
                const float* hv = hist + (lane + 1) * kQP16;
                float A = 0.0f, Bq = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j < H) {
                        A = __builtin_fmaf(pl[L.ow[6] + j], q16::qapply(hv[j] * co[j % kQP], Q.a[6]), A);
                        Bq = __builtin_fmaf(pl[L.ow[7] + j], q16::qapply(hv[j] * si[j % kQP], Q.a[7]), Bq);
                    }
                A += pl[L.ob[6]]; Bq += pl[L.ob[7]];
                yg[t0 + lane] = make_float2(A - Bq, Bq + A);
            }
        }
        wave_lds_fence();
    }
}

template <bool NW, bool DX>
__global__ __launch_bounds__(64) void bjq_bwd_kernel(SeqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, col = lane & 15, role = lane >> 4;
    const bool is_f = (role & 1) == 0;
    const BjqLayout L = bjq_layout(a.H);
    const int H = L.H, T = a.T, NC = (T + kQC - 1) / kQC;
    float* pl = smem;
    float* gw = smem + pad4(L.P);                                    // weight gradients in the parameter layout (deposited at the end)
    float4* xq = reinterpret_cast<float4*>(gw + pad4(L.P));
    float* fiq = reinterpret_cast<float*>(xq + kQX);                 // [12][64]
    float* qe = fiq + kQE * kQC;                                     // [2][64][12] q_fi(e), q_gi(e)
    float* xs = qe + 2 * kQC * kQE;                                  // [64][33] input halves; then d_f | d_g
    float* fg = xs + kQP32 * kQC;                                    // [64][33] f | g
    float* hist = fg + kQP32 * kQC;                                  // [65][17]
    float* dhh = hist + kQHist;                                      // [64][17] the read-outs' share of dL/dh(t)
    float* dcs = dhh + kQP16 * kQC;                                  // [12][64] dL/dcos_p, dL/dsin_p
    float* dfiq = dcs + kQE * kQC;                                   // [12][80] dL/dfi_p, dL/dfq_p; 64 .. 78: the later chunk's first 15 steps
    float* dyb = dfiq + kQE * kQX;                                   // [64][2]
    float* vb = dyb + 2 * kQC;                                       // [4][16] d_f, d_g, q_fh(h(t-1)), q_gh(h(t-1))
    BjqQ Q;
    qc_setup<true>(pl, a, L, Q.a, lane);
    const bool valid = col < H;
    float w[16], wT[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ow = is_f ? L.ow[3] : L.ow[5];
        w[k] = (valid && k < H) ? pl[ow + col * H + k] : 0.0f;
        wT[k] = (valid && k < H) ? pl[ow + k * H + col] : 0.0f;
    }
    for (int i = lane; i < pad4(L.P); i += 64) gw[i] = 0.0f;
    vb[lane] = 0.0f;
    // rows of unit col: W_fh | W_gh (gr), W_fi | W_gi and their bias (ge, db); lane = time step: both read-outs; lane = (filter, tap): both banks
    float gr[16], ge[kQE], db = 0.0f, dwi[16], dwq[16], tb0 = 0.0f, tb1 = 0.0f, aI0 = 0.0f, aQ0 = 0.0f, aI1 = 0.0f, aQ1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) { gr[k] = 0.0f; dwi[k] = 0.0f; dwq[k] = 0.0f; }
#pragma unroll
    for (int k = 0; k < kQE; ++k) ge[k] = 0.0f;
    const int fm = lane & 15, fp0 = lane >> 4, fp1 = 4 + ((lane >> 4) & 1);      // FIR entries (fp0, fm) and, on lanes < 32, (fp1, fm)
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        const float2* dyg = reinterpret_cast<const float2*>(a.dy) + (size_t)b * T;
        float carry = 0.0f;                                           // dL/dh of unit col from the later steps
        wave_lds_fence();
        for (int i = lane; i < kQE * kQX; i += 64) dfiq[i] = 0.0f;
        for (int c = NC - 1; c >= 0; --c) {
            const int t0 = c * kQC, len = min(kQC, T - t0);
            wave_lds_fence();
            bjq_stage_x(xq, xg, t0, T, Q, lane);
            float2 dyv = make_float2(0.0f, 0.0f);
            if (lane < len) dyv = dyg[t0 + lane];
            reinterpret_cast<float2*>(dyb)[lane] = dyv;
            wave_lds_fence();
            bjq_front<true>(pl, L, Q, xq, fiq, xs, qe, lane);
            wave_lds_fence();
            bjq_recur<true>(Q, w, xs, hist, fg, vb + 32, len, lane, valid, a.ckpt[((size_t)b * NC + c) * 16 + col]);
            // ---- the head's gradients; lane = time step ----
            {
                const bool live = lane < len;
                const float dA = dyv.x + dyv.y, dB = dyv.y - dyv.x;                       // y = (A - Bq, Bq + A)
                float co[kQP], si[kQP], dco[kQP], dsi[kQP];
#pragma unroll
                for (int p = 0; p < kQP; ++p) {
                    const BjqDemod D = bjq_demod(fiq[p * kQC + lane], fiq[(kQP + p) * kQC + lane]);
                    co[p] = D.co; si[p] = D.si; dco[p] = 0.0f; dsi[p] = 0.0f;
                }
                const float* hv = hist + (lane + 1) * kQP16;
                if constexpr (NW) { tb0 += dA; tb1 += dB; }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float dh = 0.0f;
                    if (j < H && live) {
                        const int q = j % kQP;
                        const float hj = hv[j], ir = hj * co[q], qr = hj * si[q];
                        const float dir = (dA * pl[L.ow[6] + j]) * q16::qpass(ir, Q.a[6]), dqr = (dB * pl[L.ow[7] + j]) * q16::qpass(qr, Q.a[7]);
                        if constexpr (NW) {
                            dwi[j] = __builtin_fmaf(dA, q16::qapply(ir, Q.a[6]), dwi[j]);
                            dwq[j] = __builtin_fmaf(dB, q16::qapply(qr, Q.a[7]), dwq[j]);
                        }
                        dh = __builtin_fmaf(dir, co[q], dqr * si[q]);
                        dco[q] = __builtin_fmaf(dir, hj, dco[q]);
                        dsi[q] = __builtin_fmaf(dqr, hj, dsi[q]);
                    }
                    dhh[lane * kQP16 + j] = dh;
                }
#pragma unroll
                for (int p = 0; p < kQP; ++p) { dcs[p * kQC + lane] = dco[p]; dcs[(kQP + p) * kQC + lane] = dsi[p]; }
            }
            wave_lds_fence();
            // ---- reverse recurrence; lane = unit col of row d_f | d_g | d_f | d_g ----
            {
                const float* dv = vb + (is_f ? 0 : 16);
                const float* qh = vb + (is_f ? 32 : 48);
                q16::Quant qa = Q.a[3];
                if (!is_f) qa = Q.a[5];
                for (int tt = len - 1; tt >= 0; --tt) {
                    const float hp = hist[tt * kQP16 + col], f = fg[tt * kQP32 + col], g = fg[tt * kQP32 + 16 + col];
                    const float gh = carry + dhh[tt * kQP16 + col];
                    const float dfp = valid ? (gh * (hp - g)) * (f * (1.0f - f)) : 0.0f;
                    const float dgp = valid ? (gh * (1.0f - f)) * (1.0f - g * g) : 0.0f;
                    if (role == 0) {
                        vb[col] = dfp; vb[16 + col] = dgp;
                        vb[32 + col] = q16::qapply(hp, Q.a[3]); vb[48 + col] = q16::qapply(hp, Q.a[5]);
                        xs[tt * kQP32 + col] = dfp; xs[tt * kQP32 + 16 + col] = dgp;
                    }
                    wave_lds_fence();
                    const float part = qc_dot(wT, dv, 0.0f) * q16::qpass(hp, qa);
                    const float both = part + xor16(part);      // (the swap outside the select: every lane takes part in it)
                    carry = valid ? __builtin_fmaf(gh, f, both) : 0.0f;
                    if constexpr (NW) {      // the rows of unit col: d (x) q(h(t-1)), d (x) q(e), bias
                        const float d = is_f ? dfp : dgp;
                        qc_axpy(gr, d, qh);
                        qc_axpy(ge, d, qe + ((is_f ? 0 : kQC) + tt) * kQE);
                        db += d;
                    }
                    wave_lds_fence();
                }
            }
            wave_lds_fence();
            // ---- dL/de through W_fi, W_gi (each through its layer's activation mask) and the demodulator's gradient; lane = time step ----
            {
                const bool live = lane < len;
                float def[kQE], deg[kQE];
#pragma unroll
                for (int k = 0; k < kQE; ++k) { def[k] = 0.0f; deg[k] = 0.0f; }
#pragma unroll 1
                for (int u = 0; u < H; ++u) {
                    const float df = xs[lane * kQP32 + u], dg = xs[lane * kQP32 + 16 + u];
#pragma unroll
                    for (int k = 0; k < kQE; ++k) {
                        def[k] = __builtin_fmaf(pl[L.ow[2] + u * kQE + k], df, def[k]);
                        deg[k] = __builtin_fmaf(pl[L.ow[4] + u * kQE + k], dg, deg[k]);
                    }
                }
#pragma unroll
                for (int p = 0; p < kQP; ++p) {
                    const float fi = fiq[p * kQC + lane], fq = fiq[(kQP + p) * kQC + lane];
                    const BjqDemod D = bjq_demod(fi, fq);
                    const float mag2 = D.mag * D.mag;
                    const float de1 = __builtin_fmaf(q16::qpass(D.mag, Q.a[2]), def[p], q16::qpass(D.mag, Q.a[4]) * deg[p]);
                    const float de2 = __builtin_fmaf(q16::qpass(mag2, Q.a[2]), def[kQP + p], q16::qpass(mag2, Q.a[4]) * deg[kQP + p]);
                    const float dco = dcs[p * kQC + lane], dsi = dcs[(kQP + p) * kQC + lane];
                    const float dmag = de1 + 2.0f * D.mag * de2 - (dsi * fq + dco * fi) / mag2;
                    const float im0 = D.m0 > 0.0f ? 1.0f / D.m0 : 0.0f;      // (a filter output of exactly 0: the term is dropped, as in bojanet_s16.hip)
                    const float dfi = dco / D.mag + dmag * fi * im0, dfq = dsi / D.mag + dmag * fq * im0;
                    dfiq[p * kQX + lane] = live ? dfi : 0.0f; dfiq[(kQP + p) * kQX + lane] = live ? dfq : 0.0f;
                }
            }
            wave_lds_fence();
            if constexpr (DX) {      // lane = sample s: the steps s .. s + 15 see it at tap 15 - j
                float aII = 0.0f, aQq = 0.0f, aQi = 0.0f, aIq = 0.0f;
#pragma unroll 4
                for (int j = 0; j < kQM; ++j) {
#pragma unroll
                    for (int p = 0; p < kQP; ++p) {
                        const float wI = pl[L.ow[0] + p * kQM + 15 - j], wQ = pl[L.ow[1] + p * kQM + 15 - j];
                        const float dfi = dfiq[p * kQX + lane + j], dfq = dfiq[(kQP + p) * kQX + lane + j];
                        aII = __builtin_fmaf(wI, dfi, aII); aQq = __builtin_fmaf(wQ, dfq, aQq);
                        aQi = __builtin_fmaf(wQ, dfi, aQi); aIq = __builtin_fmaf(wI, dfq, aIq);
                    }
                }
                if (lane < len) {      // fi = fir_I(I) - fir_Q(Q), fq = fir_Q(I) + fir_I(Q): every sample through both banks' activation masks
                    const float2 xv = xg[t0 + lane];
                    const float gi = __builtin_fmaf(q16::qpass(xv.x, Q.a[0]), aII, q16::qpass(xv.x, Q.a[1]) * aQq);
                    const float gq = __builtin_fmaf(q16::qpass(xv.y, Q.a[0]), aIq, -(q16::qpass(xv.y, Q.a[1]) * aQi));
                    reinterpret_cast<float2*>(a.dx)[(size_t)b * T + t0 + lane] = make_float2(gi, gq);
                }
            }
            if constexpr (NW) {      // lane = (filter, tap): d fir_I = dfi (x) q_firI(I) + dfq (x) q_firI(Q), d fir_Q = dfq (x) q_firQ(I) - dfi (x) q_firQ(Q)
                for (int tt = 0; tt < len; ++tt) {
                    const float4 v = xq[tt + 1 + fm];
                    const float i0 = dfiq[fp0 * kQX + tt], q0 = dfiq[(kQP + fp0) * kQX + tt];
                    const float i1 = dfiq[fp1 * kQX + tt], q1 = dfiq[(kQP + fp1) * kQX + tt];
                    aI0 = __builtin_fmaf(i0, v.x, __builtin_fmaf(q0, v.z, aI0)); aQ0 = __builtin_fmaf(q0, v.y, __builtin_fmaf(-i0, v.w, aQ0));
                    aI1 = __builtin_fmaf(i1, v.x, __builtin_fmaf(q1, v.z, aI1)); aQ1 = __builtin_fmaf(q1, v.y, __builtin_fmaf(-i1, v.w, aQ1));
                }
            }
            wave_lds_fence();
            if (lane < 15) {      // this chunk's first 15 steps: the halo of the earlier chunk
#pragma unroll
                for (int r = 0; r < kQE; ++r) dfiq[r * kQX + kQC + lane] = dfiq[r * kQX + lane];
            }
        }
        wave_lds_fence();
    }
    if constexpr (NW) {
        tb0 = wave_sum64(tb0); tb1 = wave_sum64(tb1);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float vi = wave_sum64(dwi[j]), vq_ = wave_sum64(dwq[j]);
            if (lane == 0 && j < H) { gw[L.ow[6] + j] = vi; gw[L.ow[7] + j] = vq_; }
        }
        if (lane == 0) { gw[L.ob[6]] = tb0; gw[L.ob[7]] = tb1; }
        if (valid && role < 2) {
            const int owh = is_f ? L.ow[3] : L.ow[5], owi = is_f ? L.ow[2] : L.ow[4], obi = is_f ? L.ob[2] : L.ob[4];
#pragma unroll
            for (int k = 0; k < 16; ++k) if (k < H) gw[owh + col * H + k] = gr[k];
#pragma unroll
            for (int k = 0; k < kQE; ++k) gw[owi + col * kQE + k] = ge[k];
            gw[obi + col] = db;
        }
        gw[L.ow[0] + fp0 * kQM + fm] = aI0; gw[L.ow[1] + fp0 * kQM + fm] = aQ0;
        if (lane < 32) { gw[L.ow[0] + fp1 * kQM + fm] = aI1; gw[L.ow[1] + fp1 * kQM + fm] = aQ1; }
        wave_lds_fence();
        qc_write_partials(a, L, gw, lane);
    }
}

}  // namespace

bool bojanet_q_ok(const odpd_model_t* m) {
    return m->backbone == ODPD_BOJANET && (m->flags & ODPD_FLAG_QUANT_CELL) && !(m->flags & (ODPD_FLAG_TWO_LAYERS | ODPD_FLAG_INIT_STATE)) &&
           qc_bits_ok(m) && m->hidden >= 1 && m->hidden <= 16;
}
int64_t bojanet_q_param_count(const odpd_model_t* m) { return bjq_layout(m->hidden).P; }      // 2H^2 + 28H + 194 + 24
int64_t bojanet_q_ckpt_floats(const odpd_model_t*, int B, int T) { return (int64_t)B * ((T + kQC - 1) / kQC) * 16; }      // h at the start of every chunk
int bojanet_q_rows(const odpd_model_t*, int B) { const int cap = 3 * device_cus(); return B < cap ? B : cap; }      // (three backward workgroups fit a CU's LDS)
int bojanet_q_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!bojanet_q_ok(m)) return ODPD_EUNSUPPORTED;
    if (a.T < kQM - 1) return ODPD_EINVAL;       // the reference cuts its 15-sample zero pad from the frame itself (bojanet.py:72-77)
    const size_t lds = (size_t)bjq_fwd_floats(bjq_layout(m->hidden).P) * sizeof(float);
    const int cap = 6 * device_cus(), grid = a.B < cap ? a.B : cap;
    return ckpt_dispatch(a, [&](auto sv) { return launch_seq(st, bjq_fwd_kernel<sv()>, grid, lds, a); });
}
int bojanet_q_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!bojanet_q_ok(m)) return ODPD_EUNSUPPORTED;
    if (a.T < kQM - 1 || !a.ckpt) return ODPD_EINVAL;
    const size_t lds = (size_t)bjq_bwd_floats(bjq_layout(m->hidden).P) * sizeof(float);
    const int grid = bojanet_q_rows(m, a.B);
    return s16_bwd_dispatch(a, [&](auto nw, auto dx) { return launch_seq(st, bjq_bwd_kernel<nw(), dx()>, grid, lds, a); });
}

}  // namespace odpd
