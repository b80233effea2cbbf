// dvrjanet_q.hip — `--quant` on dvrjanet (reference quant/quant_envs.py:40-60, 145-148, 276-306 on backbones/dvrjanet.py:5-112): all nine nn.Linear of
// the backbone — W_ph, W_ah (H -> H, no bias), W_pθ, W_ax (1 -> H, no bias), W_f (H -> H, bias), W_ccos, W_csin (2H -> H, bias), W_o1, W_o2 (H -> 1,
// bias) — become INT_Linear (quant/qmodules/quant_layers.py:48-85): each quantises ITS input on an activation grid of its own and its weight on a
// weight grid (three scale parameters behind each layer's weight / bias); `cs` stays a float parameter; atan2, sqrt, cos, sin, sigmoid, tanh, abs are
// functional and stay float; no module is named fc_out, so the 16-bit output quantiser never runs (train mode = eval mode).  Selected by
// ODPD_FLAG_QUANT_CELL on ODPD_DVRJANET with bits_w, bits_a > 0; num_dvr_units (1 .. 8) rides in the descriptor's thx.
//
// ONE sequence per single-wave workgroup (the form of bojanet_q.hip), in chunks of 64 steps.  Parameter layout, setup (the parameters staged in
// LDS with the nine weight matrices quantised IN PLACE) and write-out: odpd_qcell.h.  Per chunk:
//   front       lane = time step: |x| = sqrt(I*I + Q*Q) (two rounded products, one add: the reference's order, no FMA), theta = atan2f(Q, I), both on
//               the grid of the layer that reads them (q_ax(|x|), q_pθ(theta));
//   recurrence  lane = (role, unit), role = lane / 16; each lane keeps two weight rows in registers, block A | block B:
//                   role 0  W_ph | W_ccos[:, :H]      role 1  W_ah | W_csin[:, :H]      role 2  W_f | W_ccos[:, H:]      role 3  - | W_csin[:, H:]
//               round 1: hs = h_I + h_Q on the grids of W_ph, W_ah, W_f, h_I on W_ccos's and h_Q on W_csin's grid are broadcast through LDS; th~, the
//               DVR sum, f and the first halves of the two candidate rows; sin / cos by the straight-line sincosf_ (odpd_device.h);
//               round 2: a~ cos th~ on W_ccos's grid, a~ sin th~ on W_csin's grid broadcast; roles 2 / 3 continue the row sums of roles 0 / 1 (one
//               sum over the 2H inputs, k ascending), tanh; f, g_cos, g_sin broadcast; h' = fl(f h) + fl(fl(1 - f) g) on every lane;
//   head        lane = time step: q_o1(h_I), q_o2(h_Q), both read-outs.
// Every mat-vec sums k ascending (W8A8: products of grid values are integers below 2^14, at most 32 of them: exact in any order; W16A16 is not exact
// and this order is the kernel's own).  A value about to be rounded onto a grid is formed in the reference's operation order: th~ = fl(w q(theta)) +
// fl(W_ph q(hs)), the DVR sum 0 + |v - 1/K| c_1 + ... with the knots k/K rounded to fp32 from the double quotient; the file is compiled with FP
// contraction off.
// Backward: the chunks last to first from a checkpoint of (h_I, h_Q) per chunk — front and recurrence again (f, g_cos, g_sin, the DVR input, cos, sin
// of every step parked in LDS), the read-outs' gradients with lane = time step, the reverse recurrence with lane = (role, unit) (the transposes of
// the same two blocks in registers, every layer's activation pass mask; the weight gradients of the lane's two rows accumulate in its registers),
// dL/dtheta and dL/d|x| through both input layers' masks and on to dL/dx with lane = time step.  Sums are in a fixed order, no atomics.
// Deviation: at a sample of exactly 0 + 0j the reference's dL/dx is NaN (0 * inf through sqrt, 0 / 0 through atan2); here it is 0.
#include "odpd_qcell.h"

#pragma clang fp contract(off)

namespace odpd {
namespace {
using namespace qcell;
constexpr int kVC = 64;                             // steps per chunk
constexpr int kVP = 17;                             // row pitch of the [time][unit] buffers: conflict-free for lane = unit and for lane = time
constexpr int kVL = 9;                              // 0 W_ph  1 W_pθ  2 W_ah  3 W_ax  4 W_f  5 W_ccos  6 W_csin  7 W_o1  8 W_o2 (named_parameters order)
constexpr int kVK = 8;                              // DVR units at most
struct DvqLayout : QcLayout<kVL> { int H, K, ocs; };      // cs sits in front of the layers
__host__ __device__ inline int dvq_nin(int l, int H) { return (l == 1 || l == 3) ? 1 : (l == 5 || l == 6) ? 2 * H : H; }
__host__ __device__ inline int dvq_nout(int l, int H) { return l >= 7 ? 1 : H; }
__host__ __device__ inline DvqLayout dvq_layout(int H, int K) {
    DvqLayout L; L.H = H; L.K = K; L.ocs = 0;
    qc_fill_layout(L, K, [H](int l) { return QcLinear{dvq_nout(l, H), dvq_nin(l, H), l >= 4}; });
    return L;
}
constexpr int kVHist = ((kVC + 1) * kVP + 3) & ~3;
constexpr int kVRec = kVC * kVP;
constexpr int kVSmall = 8 * 16 + 48;                // the broadcast vectors of a forward step: eight quantised vectors; f, g_cos, g_sin
__host__ __device__ inline int dvq_fwd_floats(int P) { return pad4(P) + 2 * kVC + 2 * kVHist + kVSmall; }
__host__ __device__ inline int dvq_bwd_floats(int P) { return 2 * pad4(P) + 2 * kVC + 2 * kVHist + 8 * kVRec + kVSmall + 48 + 32 + 96; }

// what a lane of the recurrence holds besides its rows: the activation quantisers, the DVR coefficients and knots (wave-uniform), its own scalars
struct DvqQ {
    q16::Quant a[kVL];
    float cs[kVK], knot[kVK];
    int K;
};
// the shared setup, then the DVR coefficients (cs is no layer's weight: the staged copy keeps it as it is) and knots
__device__ __forceinline__ void dvq_setup(float* pl, const SeqArgs& a, const DvqLayout& L, DvqQ& Q, int lane) {
    qc_setup<true>(pl, a, L, Q.a, lane);
    Q.K = L.K;
#pragma unroll
    for (int k = 0; k < kVK; ++k) {
        Q.cs[k] = k < L.K ? uni_(pl[L.ocs + (k < L.K ? k : 0)]) : 0.0f;
        Q.knot[k] = (float)((double)(k + 1) / (double)L.K);      // (dvrjanet.py:38: the Python float k / num_k, rounded when it meets the fp32 tensor)
    }
}
// a lane's choice among layout offsets / quantisers, made on values that are already loaded (a choice between two loads of the layout can come out
// as one load from a chosen address, which puts the whole layout into scratch)
__device__ __forceinline__ int dvq_pick(int role, int v0, int v1, int v2, int v3) { return role == 0 ? v0 : role == 1 ? v1 : role == 2 ? v2 : v3; }
__device__ __forceinline__ q16::Quant dvq_pick(int role, q16::Quant v0, q16::Quant v1, q16::Quant v2, q16::Quant v3) {
    q16::Quant q;
    q.s = role == 0 ? v0.s : role == 1 ? v1.s : role == 2 ? v2.s : v3.s;
    q.inv = role == 0 ? v0.inv : role == 1 ? v1.inv : role == 2 ? v2.inv : v3.inv;
    q.qn = v0.qn; q.qp = v0.qp;      // (one activation bit width for every layer)
    return q;
}
// the DVR block (dvrjanet.py:32-41): 0 + |v - 1/K| c_1 + ... in ascending k, each term a rounded product; sg: sum of c_k sign(v - k/K) (abs has slope 0 at 0)
__device__ __forceinline__ float dvq_dvr(const DvqQ& Q, float v, float& sg) {
    float at = 0.0f;
    sg = 0.0f;
#pragma unroll
    for (int k = 0; k < kVK; ++k)
        if (k < Q.K) {
            const float d = v - Q.knot[k];
            at = at + __builtin_fabsf(d) * Q.cs[k];
            sg += d > 0.0f ? Q.cs[k] : d < 0.0f ? -Q.cs[k] : 0.0f;
        }
    return at;
}
// the rows of lane (role, col): block A | block B of the table above (tr: their transposes — column col of the block)
__device__ __forceinline__ void dvq_rows(const float* pl, const DvqLayout& L, int role, int col, bool tr, float (&wA)[16], float (&wB)[16]) {
    const int H = L.H;
    const int oa = dvq_pick(role, L.ow[0], L.ow[2], L.ow[4], L.ow[4]);
    const int obk = dvq_pick(role, L.ow[5], L.ow[6], L.ow[5], L.ow[6]) + (role >= 2 ? H : 0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool in = col < H && k < H;
        wA[k] = (in && role < 3) ? pl[oa + (tr ? k * H + col : col * H + k)] : 0.0f;
        wB[k] = in ? pl[obk + (tr ? k * 2 * H + col : col * 2 * H + k)] : 0.0f;
    }
}
// front of the chunk, lane = time step: |x| and theta on the grids of the layers that read them -> io[0..63] = q_pθ(theta), io[64..127] = q_ax(|x|)
__device__ __forceinline__ void dvq_front(const DvqQ& Q, float* io, float2 xv, float& mag, float& theta, int lane) {
    mag = sqrtf(xv.x * xv.x + xv.y * xv.y);
    theta = atan2f(xv.y, xv.x);
    io[lane] = q16::qapply(theta, Q.a[1]);
    io[kVC + lane] = q16::qapply(mag, Q.a[3]);
}
// the recurrence over the chunk's steps: entry tt + 1 of histI / histQ = the state after step t0 + tt; SV: f, g_cos, g_sin, the DVR input, cos, sin
// of every step parked in rec[0..5]
// vq: [8][16] broadcast vectors — 0 q_ph(hs)  1 q_ah(hs)  2 q_f(hs)  3 unused  4 q_ccos(h_I)  5 q_csin(h_Q)  6 q_ccos(a~ cos)  7 q_csin(a~ sin);  ex: [3][16] f, g_cos, g_sin
template <bool SV>
__device__ __forceinline__ void dvq_recur(const DvqQ& Q, const float (&wA)[16], const float (&wB)[16], float sc, float bA, float bB, const float* io,
                                          float* histI, float* histQ, float* rec, float* vq, float* ex, int len, int lane, bool valid, float& hI,
                                          float& hQ) {
    const int col = lane & 15, role = lane >> 4;
    const q16::Quant qa = dvq_pick(role, Q.a[0], Q.a[2], Q.a[4], Q.a[4]), qb = dvq_pick(role, Q.a[5], Q.a[6], Q.a[5], Q.a[6]);
    if (role == 0) { histI[col] = hI; histQ[col] = hQ; }
    for (int tt = 0; tt < len; ++tt) {
        const float hs = hI + hQ;
        vq[role * 16 + col] = q16::qapply(hs, qa);
        if (role < 2) vq[(4 + role) * 16 + col] = q16::qapply(role == 0 ? hI : hQ, qb);
        wave_lds_fence();
        const float accA = qc_dot(wA, vq + role * 16, 0.0f);
        float accB = 0.0f;
        if (role < 2) accB = qc_dot(wB, vq + (4 + role) * 16, 0.0f);
        // role 0: th~ and its sin / cos; role 1: the DVR input and sum; role 2: f
        const float pre = sc * io[(role & 1) * kVC + tt] + accA;
        float si, co, sg;
        sincosf_(pre, si, co);
        const float at = dvq_dvr(Q, pre, sg);
        const float f0 = sigmoidf_(accA + bA);
        const float co1 = xor16(co), si1 = xor16(si);      // role 1 receives role 0's
        if (role == 1) {
            vq[6 * 16 + col] = q16::qapply(at * co1, Q.a[5]);
            vq[7 * 16 + col] = q16::qapply(at * si1, Q.a[6]);
            if constexpr (SV) { rec[3 * kVRec + tt * kVP + col] = pre; rec[4 * kVRec + tt * kVP + col] = co1; rec[5 * kVRec + tt * kVP + col] = si1; }
        }
        const float part = __shfl_xor(accB, 32);            // roles 2 / 3 continue the sums of roles 0 / 1
        wave_lds_fence();
        if (role >= 2) {
            const float g0 = tanhf_(qc_dot(wB, vq + (4 + role) * 16, part) + bB);
            if (role == 2) { ex[col] = f0; ex[16 + col] = g0; }
            else ex[32 + col] = g0;
        }
        wave_lds_fence();
        const float f = ex[col], gc = ex[16 + col], gs = ex[32 + col];
        const float nf = 1.0f - f;
        hI = valid ? f * hI + nf * gc : 0.0f;
        hQ = valid ? f * hQ + nf * gs : 0.0f;
        if (role == 0) {
            histI[(tt + 1) * kVP + col] = hI; histQ[(tt + 1) * kVP + col] = hQ;
            if constexpr (SV) { rec[tt * kVP + col] = f; rec[kVRec + tt * kVP + col] = gc; rec[2 * kVRec + tt * kVP + col] = gs; }
        }
    }
    wave_lds_fence();
}
// the per-lane scalars of the recurrence: sc = the lane's entry of w_pθ (role 0) / w_ax (role 1); bA = b_f (role 2); bB = b_ccos (role 2) / b_csin (role 3)
__device__ __forceinline__ void dvq_scalars(const float* pl, const DvqLayout& L, int role, int col, float& sc, float& bA, float& bB) {
    const bool valid = col < L.H;
    const int osc = dvq_pick(role, L.ow[1], L.ow[3], L.ow[1], L.ow[3]), obb = dvq_pick(role, L.ob[5], L.ob[6], L.ob[5], L.ob[6]), obf = L.ob[4];
    sc = (valid && role < 2) ? pl[osc + col] : 0.0f;
    bA = (valid && role == 2) ? pl[obf + col] : 0.0f;
    bB = (valid && role >= 2) ? pl[obb + col] : 0.0f;
}

template <bool SAVE>
__global__ __launch_bounds__(64) void dvq_fwd_kernel(SeqArgs a, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, col = lane & 15, role = lane >> 4;
    const DvqLayout L = dvq_layout(a.H, K);
    const int H = L.H, T = a.T, NC = (T + kVC - 1) / kVC;
    float* pl = smem;
    float* io = smem + pad4(L.P);                                    // [2][64] q_pθ(theta), q_ax(|x|)
    float* histI = io + 2 * kVC;                                     // [65][17]
    float* histQ = histI + kVHist;
    float* vq = histQ + kVHist;                                      // [8][16]
    float* ex = vq + 8 * 16;                                         // [3][16]
    DvqQ Q;
    dvq_setup(pl, a, L, Q, lane);
    const bool valid = col < H;
    float wA[16], wB[16], sc, bA, bB;
    dvq_rows(pl, L, role, col, false, wA, wB);
    dvq_scalars(pl, L, role, col, sc, bA, bB);
    for (int i = lane; i < kVSmall; i += 64) vq[i] = 0.0f;
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        float2* yg = reinterpret_cast<float2*>(a.y) + (size_t)b * T;
        float hI = 0.0f, hQ = 0.0f;
        for (int c = 0; c < NC; ++c) {
            const int t0 = c * kVC, len = min(kVC, T - t0);
            if constexpr (SAVE) {
                if (role < 2) a.ckpt[((size_t)b * NC + c) * 32 + role * 16 + col] = role == 0 ? hI : hQ;
            }
            wave_lds_fence();
            float mag, theta;
            dvq_front(Q, io, lane < len ? xg[t0 + lane] : make_float2(0.5f, 0.5f), mag, theta, lane);
            wave_lds_fence();
            dvq_recur<false>(Q, wA, wB, sc, bA, bB, io, histI, histQ, nullptr, vq, ex, len, lane, valid, hI, hQ);
            if (lane < len) {      // the chunk's outputs, lane = time step
                const float* hi = histI + (lane + 1) * kVP;
                const float* hq = histQ + (lane + 1) * kVP;
                float A = 0.0f, Bq = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j < H) {
                        A = __builtin_fmaf(pl[L.ow[7] + j], q16::qapply(hi[j], Q.a[7]), A);
                        Bq = __builtin_fmaf(pl[L.ow[8] + j], q16::qapply(hq[j], Q.a[8]), Bq);
                    }
                A += pl[L.ob[7]]; Bq += pl[L.ob[8]];
                yg[t0 + lane] = make_float2(A, Bq);
            }
        }
        wave_lds_fence();
    }
}

template <bool NW, bool DX>
__global__ __launch_bounds__(64) void dvq_bwd_kernel(SeqArgs a, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, col = lane & 15, role = lane >> 4;
    const DvqLayout L = dvq_layout(a.H, K);
    const int H = L.H, T = a.T, NC = (T + kVC - 1) / kVC;
    float* pl = smem;
    float* gw = smem + pad4(L.P);                                    // weight gradients in the parameter layout (deposited at the end)
    float* io = gw + pad4(L.P);                                      // [2][64] q_pθ(theta), q_ax(|x|)
    float* histI = io + 2 * kVC;                                     // [65][17]
    float* histQ = histI + kVHist;
    float* rec = histQ + kVHist;                                     // [6][64][17] f, g_cos, g_sin, DVR input, cos, sin; rows 0 / 1 become dL/dth~, dL/d(DVR input) in the reverse pass
    float* dhh = rec + 6 * kVRec;                                    // [2][64][17] the read-outs' share of dL/dh_I(t), dL/dh_Q(t)
    float* vq = dhh + 2 * kVRec;                                     // [8][16]
    float* ex = vq + 8 * 16;                                         // [3][16]
    float* db = ex + 48;                                             // [3][16] dL/d(pre-activation) of f, g_cos, g_sin
    float* dv = db + 48;                                             // [2][16] dL/dth~, dL/d(DVR input)
    float* comb = dv + 32;                                           // [6][16] the roles' shares of dL/dhs (0 .. 3), of dL/dh_I (4), dL/dh_Q (5)
    DvqQ Q;
    dvq_setup(pl, a, L, Q, lane);
    const bool valid = col < H;
    float wA[16], wB[16], tA[16], tB[16], sc, bA, bB;
    dvq_rows(pl, L, role, col, false, wA, wB);
    dvq_rows(pl, L, role, col, true, tA, tB);
    dvq_scalars(pl, L, role, col, sc, bA, bB);
    for (int i = lane; i < pad4(L.P); i += 64) gw[i] = 0.0f;
    for (int i = lane; i < kVSmall + 48 + 32 + 96; i += 64) vq[i] = 0.0f;
    // the lane's two rows (gA, gB), its entry of w_pθ / w_ax (gsc) and of the biases (gbA, gbB); role 2: cs; lane = time step: both read-outs
    float gA[16], gB[16], gsc = 0.0f, gbA = 0.0f, gbB = 0.0f, dcs[kVK], dw1[16], dw2[16], tb0 = 0.0f, tb1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) { gA[k] = 0.0f; gB[k] = 0.0f; dw1[k] = 0.0f; dw2[k] = 0.0f; }
#pragma unroll
    for (int k = 0; k < kVK; ++k) dcs[k] = 0.0f;
    // the pass masks a lane applies: to hs on its block A's grid, to h_I / h_Q (roles 0 / 1) or a~ cos / a~ sin (roles 2 / 3) on its block B's grid
    const q16::Quant qa = dvq_pick(role, Q.a[0], Q.a[2], Q.a[4], Q.a[4]), qb = dvq_pick(role, Q.a[5], Q.a[6], Q.a[5], Q.a[6]);
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        const float2* dyg = reinterpret_cast<const float2*>(a.dy) + (size_t)b * T;
        float cI = 0.0f, cQ = 0.0f;                                   // dL/dh_I, dL/dh_Q of unit col from the later steps
        for (int c = NC - 1; c >= 0; --c) {
            const int t0 = c * kVC, len = min(kVC, T - t0);
            const bool live = lane < len;
            wave_lds_fence();
            const float2 xv = live ? xg[t0 + lane] : make_float2(0.5f, 0.5f);
            float mag, theta;
            dvq_front(Q, io, xv, mag, theta, lane);
            float2 dyv = make_float2(0.0f, 0.0f);
            if (live) dyv = dyg[t0 + lane];
            wave_lds_fence();
            {
                const float* ck = a.ckpt + ((size_t)b * NC + c) * 32;
                float hI = ck[col], hQ = ck[16 + col];
                dvq_recur<true>(Q, wA, wB, sc, bA, bB, io, histI, histQ, rec, vq, ex, len, lane, valid, hI, hQ);
            }
            // ---- the read-outs' gradients; lane = time step ----
            {
                const float* hi = histI + (lane + 1) * kVP;
                const float* hq = histQ + (lane + 1) * kVP;
                if constexpr (NW) { tb0 += dyv.x; tb1 += dyv.y; }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float d1 = 0.0f, d2 = 0.0f;
                    if (j < H && live) {
                        const float a1 = hi[j], a2 = hq[j];
                        d1 = (dyv.x * pl[L.ow[7] + j]) * q16::qpass(a1, Q.a[7]);
                        d2 = (dyv.y * pl[L.ow[8] + j]) * q16::qpass(a2, Q.a[8]);
                        if constexpr (NW) {
                            dw1[j] = __builtin_fmaf(dyv.x, q16::qapply(a1, Q.a[7]), dw1[j]);
                            dw2[j] = __builtin_fmaf(dyv.y, q16::qapply(a2, Q.a[8]), dw2[j]);
                        }
                    }
                    dhh[lane * kVP + j] = d1; dhh[kVRec + lane * kVP + j] = d2;
                }
            }
            wave_lds_fence();
            // ---- reverse recurrence; lane = (role, unit) ----
            for (int tt = len - 1; tt >= 0; --tt) {
                const int r = tt * kVP + col;
                const float hIp = histI[r], hQp = histQ[r], f = rec[r], gc = rec[kVRec + r], gs = rec[2 * kVRec + r];
                const float ap = rec[3 * kVRec + r], co = rec[4 * kVRec + r], si = rec[5 * kVRec + r];
                const float hs = hIp + hQp;
                const float gI = cI + dhh[r], gQ = cQ + dhh[kVRec + r];
                const float nf = 1.0f - f;
                const float dpf = valid ? (gI * (hIp - gc) + gQ * (hQp - gs)) * (f * nf) : 0.0f;
                const float dpc = valid ? (gI * nf) * (1.0f - gc * gc) : 0.0f;
                const float dps = valid ? (gQ * nf) * (1.0f - gs * gs) : 0.0f;
                float sg;
                const float at = dvq_dvr(Q, ap, sg);
                const float vb = (role & 1) ? (role == 1 ? hQp : at * si) : (role == 0 ? hIp : at * co);      // what the lane's block B read at unit col
                if (role == 0) { db[col] = dpf; db[16 + col] = dpc; db[32 + col] = dps; }
                if constexpr (NW) {
                    vq[role * 16 + col] = q16::qapply(hs, qa);
                    vq[(4 + role) * 16 + col] = q16::qapply(vb, qb);
                }
                wave_lds_fence();
                const float dB = (role & 1) ? dps : dpc;
                // round 1: block B's transpose on dL/d(g_cos pre) / dL/d(g_sin pre); role 2: W_f's on dL/d(f pre)
                const float mB = qc_dot(tB, db + ((role & 1) ? 32 : 16), 0.0f) * q16::qpass(vb, qb);
                float mA = 0.0f;
                if (role == 2) mA = qc_dot(tA, db, 0.0f) * q16::qpass(hs, qa);
                const float dvs = xor16(mB);                          // role 2 holds dL/d(a~ cos), receives dL/d(a~ sin) from role 3
                const float dat = mB * co + dvs * si;
                const float dth = at * (dvs * co - mB * si), dap = dat * sg;
                if (role == 2) {
                    dv[col] = dth; dv[16 + col] = dap;
                    rec[r] = dth; rec[kVRec + r] = dap;               // (f, g_cos of this step are in registers by now)
                    if constexpr (NW) {
#pragma unroll
                        for (int k = 0; k < kVK; ++k)
                            if (k < Q.K) dcs[k] = __builtin_fmaf(dat, __builtin_fabsf(ap - Q.knot[k]), dcs[k]);
                    }
                }
                wave_lds_fence();
                // round 2: W_ph's transpose on dL/dth~ (role 0), W_ah's on dL/d(DVR input) (role 1)
                if (role < 2) mA = qc_dot(tA, dv + role * 16, 0.0f) * q16::qpass(hs, qa);
                comb[role * 16 + col] = mA;
                if (role < 2) comb[(4 + role) * 16 + col] = mB;
                wave_lds_fence();
                const float dhs = (comb[col] + comb[16 + col]) + comb[32 + col];
                cI = valid ? __builtin_fmaf(gI, f, dhs + comb[64 + col]) : 0.0f;
                cQ = valid ? __builtin_fmaf(gQ, f, dhs + comb[80 + col]) : 0.0f;
                if constexpr (NW) {      // the lane's rows: d (x) q(input), its input-column entry, its biases
                    const float dA = role == 2 ? dpf : role < 2 ? dv[role * 16 + col] : 0.0f;
                    qc_axpy(gA, dA, vq + role * 16);
                    qc_axpy(gB, dB, vq + (4 + role) * 16);
                    gsc = __builtin_fmaf(dA, io[(role & 1) * kVC + tt], gsc);
                    gbA += dA; gbB += dB;
                }
                wave_lds_fence();
            }
            // ---- dL/dtheta, dL/d|x| through the input layers' masks, on to dL/dx; lane = time step ----
            if constexpr (DX) {
                float st = 0.0f, sm = 0.0f;
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    if (u < H) {
                        st = __builtin_fmaf(pl[L.ow[1] + u], rec[lane * kVP + u], st);
                        sm = __builtin_fmaf(pl[L.ow[3] + u], rec[kVRec + lane * kVP + u], sm);
                    }
                if (live) {
                    const float dth = st * q16::qpass(theta, Q.a[1]), dmg = sm * q16::qpass(mag, Q.a[3]);
                    const float r2 = xv.x * xv.x + xv.y * xv.y;
                    float gi = 0.0f, gq = 0.0f;
                    if (r2 > 0.0f) {      // (a sample of exactly 0: the reference's NaN is dropped)
                        const float im = dmg / mag, ir = dth / r2;
                        gi = im * xv.x - ir * xv.y; gq = im * xv.y + ir * xv.x;
                    }
                    reinterpret_cast<float2*>(a.dx)[(size_t)b * T + t0 + lane] = make_float2(gi, gq);
                }
            }
        }
        wave_lds_fence();
    }
    if constexpr (NW) {
        tb0 = wave_sum64(tb0); tb1 = wave_sum64(tb1);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v1 = wave_sum64(dw1[j]), v2 = wave_sum64(dw2[j]);
            if (lane == 0 && j < H) { gw[L.ow[7] + j] = v1; gw[L.ow[8] + j] = v2; }
        }
#pragma unroll
        for (int k = 0; k < kVK; ++k) {
            const float v = wave_sum64(role == 2 ? dcs[k] : 0.0f);
            if (lane == 0 && k < L.K) gw[L.ocs + k] = v;
        }
        if (lane == 0) { gw[L.ob[7]] = tb0; gw[L.ob[8]] = tb1; }
        if (valid) {
            const int oa = dvq_pick(role, L.ow[0], L.ow[2], L.ow[4], L.ow[4]);
            const int obk = dvq_pick(role, L.ow[5], L.ow[6], L.ow[5], L.ow[6]) + (role >= 2 ? H : 0);
            const int osc = dvq_pick(role, L.ow[1], L.ow[3], L.ow[1], L.ow[3]), obb = dvq_pick(role, L.ob[5], L.ob[6], L.ob[5], L.ob[6]), obf = L.ob[4];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < H) {
                    if (role < 3) gw[oa + col * H + k] = gA[k];
                    gw[obk + col * 2 * H + k] = gB[k];
                }
            if (role < 2) gw[osc + col] = gsc;
            if (role == 2) gw[obf + col] = gbA;
            if (role >= 2) gw[obb + col] = gbB;
        }
        wave_lds_fence();
        qc_write_partials(a, L, gw, lane);
    }
}

// num_dvr_units rides in thx as an exact small integer (thx / thh are otherwise the delta backbones' thresholds); 0: not one
inline int dvq_units(const odpd_model_t* m) {
    const int K = (int)m->thx;
    return ((float)K == m->thx && K >= 1 && K <= kVK && m->thh == 0.0f) ? K : 0;
}
}  // namespace

bool dvrjanet_q_ok(const odpd_model_t* m) {
    return m->backbone == ODPD_DVRJANET && (m->flags & ODPD_FLAG_QUANT_CELL) && !(m->flags & (ODPD_FLAG_TWO_LAYERS | ODPD_FLAG_INIT_STATE)) &&
           qc_bits_ok(m) && m->hidden >= 1 && m->hidden <= 16 && dvq_units(m) > 0;
}
int64_t dvrjanet_q_param_count(const odpd_model_t* m) { return dvq_layout(m->hidden, dvq_units(m)).P; }      // K + 7H^2 + 7H + 2 + 27
int64_t dvrjanet_q_ckpt_floats(const odpd_model_t*, int B, int T) { return (int64_t)B * ((T + kVC - 1) / kVC) * 32; }      // (h_I, h_Q) at the start of every chunk
int dvrjanet_q_rows(const odpd_model_t*, int B) { const int cap = 2 * device_cus(); return B < cap ? B : cap; }      // (two backward workgroups fit a CU's LDS)
int dvrjanet_q_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!dvrjanet_q_ok(m)) return ODPD_EUNSUPPORTED;
    const int K = dvq_units(m);
    const size_t lds = (size_t)dvq_fwd_floats(dvq_layout(m->hidden, K).P) * sizeof(float);
    const int cap = 8 * device_cus(), grid = a.B < cap ? a.B : cap;
    return ckpt_dispatch(a, [&](auto sv) { return launch_seq(st, dvq_fwd_kernel<sv()>, grid, lds, a, K); });
}
int dvrjanet_q_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!dvrjanet_q_ok(m)) return ODPD_EUNSUPPORTED;
    if (!a.ckpt) return ODPD_EINVAL;
    const int K = dvq_units(m);
    const size_t lds = (size_t)dvq_bwd_floats(dvq_layout(m->hidden, K).P) * sizeof(float);
    const int grid = dvrjanet_q_rows(m, a.B);
    return s16_bwd_dispatch(a, [&](auto nw, auto dx) { return launch_seq(st, dvq_bwd_kernel<nw(), dx()>, grid, lds, a, K); });
}

}  // namespace odpd
