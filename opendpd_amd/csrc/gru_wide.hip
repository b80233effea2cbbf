// gru_wide.hip — gru / dgru / qgru / qgru_amp1 with 33 .. 64 hidden units (one layer; reference: backbones/gru.py:4-48, dgru.py:9-74,
// qgru.py:9-71, qgru_amp1.py:9-76 — `hidden_size` is a free argument of all four, arguments.py:49-60): ONE sequence per single-wave workgroup,
// LANE = HIDDEN UNIT.  The 16-wide tile kernels (gru_family.hip, gru_s16*.hip) stop at two unit tiles; here a unit's three W_hh rows (3 x 64
// registers) stay with its lane, the state is broadcast through LDS once per step (16 x ds_read_b128 of one address), and what does not depend
// on the recurrence runs with lane = time step on 64-step chunks (features; heads: fc_out, or dgru's fc_hid + relu + fc_out over [hid, features]).
//   forward   r, z, n, W_hn h + b_hn and h of every step (dgru: + the fc_hid pre-activation) go to a per-sequence record in HBM (the `ckpt`
//             buffer: B x T x NS x 64 floats) when the backward pass is going to need them;
//   backward  chunks in reverse; per step the lane of unit k forms dL/dh(t-1)[k] from the step's gate gradients (broadcast through LDS) and
//             column k of W_hh (read from the staged parameters: consecutive lanes, consecutive addresses); dW_hh accumulates as outer
//             products on the 4-block MFMA (v_mfma_f32_16x16x1_4b_f32: block b = units 16b .., the state rotated by 0 / 16 / 32 / 48 lanes
//             supplies the four column blocks), dW_ih and the biases on the VALU; dgru: the head's gradients of a chunk are formed with
//             lane = time step (dL/dhid, fc_hid^T dL/dhid -> dL/dh, the feature columns of fc_out), dW_hid as 16 x 16 x 4 MFMA tiles over the
//             chunk's (dL/dhid, h) rows in LDS.  One row of partial gradients per workgroup (every entry written).
// These kernels serve the shapes the tile kernels do not; they are built for correctness and a sane step time (LDS-broadcast bound, about
// 0.2 .. 0.4 us per time step and sequence), not for the roofline.
// The state route (ODPD_FLAG_INIT_STATE: odpd_backbone_fwd_state / _bwd_state, 1 .. 64 hidden units) runs the same bodies with S0 set: a
// sequence starts from h0[b][unit] instead of 0 (lanes >= H keep 0), the backward sees h0 as h(-1) and writes the dL/dh(-1) it carries out
// of step 0 to dh0[b][unit].  Below 33 units whole 16-unit blocks are padding: their states, gate gradients and weights are zero, and the
// partial-gradient writes skip them (ju, ku < H).  Each body is spelled out inside both kernels (#include of gru_wide_{fwd,bwd}_body.h):
// the S0 = false kernels then compile to the instructions they had before the state route existed, which an inlined __device__ body
// shared by the two does not give (it schedules and allocates them differently).
#include "odpd_seq.h"

namespace odpd {
namespace {
constexpr int kWC = 64;          // time steps per chunk
constexpr int kWS = 65;          // row stride of the per-chunk [time][unit] arrays (lane = unit and lane = time accesses both conflict-free)
constexpr int kWHs = ((kWC + 1) * kWS + 3) & ~3;      // floats of the [65][65] state array, padded so that what follows stays 16-byte aligned

template <int FM>
__device__ __forceinline__ void wide_stage_features(float* ftab, const float2* xg, int t0, int T, int lane) {
    constexpr int F = FeatDim<FM>::F;
    const int t = t0 + lane;
    const float2 xv = t < T ? xg[t] : make_float2(0.5f, 0.5f);
    float f[F], o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    feat_fwd<FM>(xv.x, xv.y, f);
#pragma unroll
    for (int i = 0; i < F; ++i) o[i] = f[i];
    reinterpret_cast<float4*>(ftab)[2 * lane] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<float4*>(ftab)[2 * lane + 1] = make_float4(o[4], o[5], o[6], o[7]);
}
__host__ __device__ inline int wide_fwd_floats(int P, bool dg, int H) {
    return pad4(P) + kWC * 8 + 64 + kWC * kWS + (dg ? kWC * kWS + H * 64 : 0);
}
__host__ __device__ inline int wide_bwd_floats(int P, bool dg, int H) {
    return pad4(P) + kWC * 8 + kWC * 8 + kWC * 2 + 4 * 64 + kWHs + (dg ? 2 * kWC * kWS + H * 64 : 0);
}

template <int FM, bool DG, bool SAVE>
__global__ __launch_bounds__(64) void wide_gru_fwd_kernel(SeqArgs a) {
    constexpr bool S0 = false;
#include "gru_wide_fwd_body.h"
}
template <int FM, bool DG, bool SAVE>
__global__ __launch_bounds__(64) void wide_gru_fwd_state_kernel(SeqArgs a) {
    constexpr bool S0 = true;
#include "gru_wide_fwd_body.h"
}

template <int FM, bool DG, bool NW, bool DX>
__global__ __launch_bounds__(64) void wide_gru_bwd_kernel(SeqArgs a) {
    constexpr bool S0 = false;
#include "gru_wide_bwd_body.h"
}
template <int FM, bool DG, bool NW, bool DX>
__global__ __launch_bounds__(64) void wide_gru_bwd_state_kernel(SeqArgs a) {
    constexpr bool S0 = true;
#include "gru_wide_bwd_body.h"
}

bool wide_cfg(const odpd_model_t* m, int& FM, bool& DG) {
    switch (m->backbone) {
    case ODPD_GRU: FM = FEAT_RAW2; DG = false; return true;
    case ODPD_DGRU: FM = FEAT_DGRU6; DG = true; return true;
    case ODPD_QGRU: FM = FEAT_Q4; DG = false; return true;
    case ODPD_QGRU_AMP1: FM = FEAT_A4; DG = false; return true;
    default: return false;
    }
}
int wide_P(const odpd_model_t* m, int FM, bool DG) { return gru_layout(m->hidden, FM == FEAT_RAW2 ? 2 : (FM == FEAT_DGRU6 ? 6 : 4), DG).P; }
}  // namespace

// float gru / dgru / qgru / qgru_amp1 of 33 .. 64 hidden units
bool gru_wide_ok(const odpd_model_t* m) {
    int FM; bool DG;
    return m->bits_w == 0 && m->hidden > 32 && m->hidden <= 64 && wide_cfg(m, FM, DG);
}
int64_t gru_wide_ckpt_floats(const odpd_model_t* m, int B, int T) { return (int64_t)B * T * (m->backbone == ODPD_DGRU ? 6 : 5) * 64; }
int gru_wide_rows(const odpd_model_t*, int B) { const int cap = 4 * device_cus(); return B < cap ? B : cap; }
int gru_wide_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    int FM; bool DG;
    if (!gru_wide_ok(m) || !wide_cfg(m, FM, DG)) return ODPD_EUNSUPPORTED;
    const size_t lds = (size_t)wide_fwd_floats(wide_P(m, FM, DG), DG, m->hidden) * sizeof(float);
    const int grid = gru_wide_rows(m, a.B);
#define ODPD_WIDE_FWD(FM_, DG_) \
    if (FM == FM_) return a.ckpt ? launch_seq(st, wide_gru_fwd_kernel<FM_, DG_, true>, grid, lds, a) : launch_seq(st, wide_gru_fwd_kernel<FM_, DG_, false>, grid, lds, a);
    ODPD_WIDE_FWD(FEAT_RAW2, false) ODPD_WIDE_FWD(FEAT_DGRU6, true) ODPD_WIDE_FWD(FEAT_Q4, false) ODPD_WIDE_FWD(FEAT_A4, false)
#undef ODPD_WIDE_FWD
    return ODPD_EUNSUPPORTED;
}
int gru_wide_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    int FM; bool DG;
    if (!gru_wide_ok(m) || !wide_cfg(m, FM, DG)) return ODPD_EUNSUPPORTED;
    if (!a.ckpt) return ODPD_EINVAL;
    const size_t lds = (size_t)wide_bwd_floats(wide_P(m, FM, DG), DG, m->hidden) * sizeof(float);
    const int grid = gru_wide_rows(m, a.B);
    const bool nw = a.partials != nullptr, dx = a.dx != nullptr;
#define ODPD_WIDE_BWD(FM_, DG_)                                                                              \
    if (FM == FM_) {                                                                                         \
        if (nw && dx) return launch_seq(st, wide_gru_bwd_kernel<FM_, DG_, true, true>, grid, lds, a);        \
        if (nw) return launch_seq(st, wide_gru_bwd_kernel<FM_, DG_, true, false>, grid, lds, a);             \
        return launch_seq(st, wide_gru_bwd_kernel<FM_, DG_, false, true>, grid, lds, a);                     \
    }
    ODPD_WIDE_BWD(FEAT_RAW2, false) ODPD_WIDE_BWD(FEAT_DGRU6, true) ODPD_WIDE_BWD(FEAT_Q4, false) ODPD_WIDE_BWD(FEAT_A4, false)
#undef ODPD_WIDE_BWD
    return ODPD_EUNSUPPORTED;
}

// the state route: float gru / dgru / qgru / qgru_amp1 of 1 .. 64 hidden units, one layer, from a caller-given initial state (a.h0)
bool gru_state_ok(const odpd_model_t* m) {
    int FM; bool DG;
    return m->bits_w == 0 && m->hidden >= 1 && m->hidden <= 64 && !(m->flags & ODPD_FLAG_TWO_LAYERS) && wide_cfg(m, FM, DG);
}
int gru_state_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    int FM; bool DG;
    if (!gru_state_ok(m) || !wide_cfg(m, FM, DG)) return ODPD_EUNSUPPORTED;
    if (!a.h0) return ODPD_EINVAL;
    const size_t lds = (size_t)wide_fwd_floats(wide_P(m, FM, DG), DG, m->hidden) * sizeof(float);
    const int grid = gru_wide_rows(m, a.B);
#define ODPD_STATE_FWD(FM_, DG_) \
    if (FM == FM_) return a.ckpt ? launch_seq(st, wide_gru_fwd_state_kernel<FM_, DG_, true>, grid, lds, a) : launch_seq(st, wide_gru_fwd_state_kernel<FM_, DG_, false>, grid, lds, a);
    ODPD_STATE_FWD(FEAT_RAW2, false) ODPD_STATE_FWD(FEAT_DGRU6, true) ODPD_STATE_FWD(FEAT_Q4, false) ODPD_STATE_FWD(FEAT_A4, false)
#undef ODPD_STATE_FWD
    return ODPD_EUNSUPPORTED;
}
int gru_state_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    int FM; bool DG;
    if (!gru_state_ok(m) || !wide_cfg(m, FM, DG)) return ODPD_EUNSUPPORTED;
    if (!a.ckpt || !a.h0) return ODPD_EINVAL;
    const size_t lds = (size_t)wide_bwd_floats(wide_P(m, FM, DG), DG, m->hidden) * sizeof(float);
    const int grid = gru_wide_rows(m, a.B);
    const bool nw = a.partials != nullptr, dx = a.dx != nullptr;      // (neither: dL/dh0 alone)
#define ODPD_STATE_BWD(FM_, DG_)                                                                                   \
    if (FM == FM_) {                                                                                               \
        if (nw && dx) return launch_seq(st, wide_gru_bwd_state_kernel<FM_, DG_, true, true>, grid, lds, a);        \
        if (nw) return launch_seq(st, wide_gru_bwd_state_kernel<FM_, DG_, true, false>, grid, lds, a);             \
        if (dx) return launch_seq(st, wide_gru_bwd_state_kernel<FM_, DG_, false, true>, grid, lds, a);             \
        return launch_seq(st, wide_gru_bwd_state_kernel<FM_, DG_, false, false>, grid, lds, a);                    \
    }
    ODPD_STATE_BWD(FEAT_RAW2, false) ODPD_STATE_BWD(FEAT_DGRU6, true) ODPD_STATE_BWD(FEAT_Q4, false) ODPD_STATE_BWD(FEAT_A4, false)
#undef ODPD_STATE_BWD
    return ODPD_EUNSUPPORTED;
}

}  // namespace odpd
