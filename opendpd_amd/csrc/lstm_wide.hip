// lstm_wide.hip — the plain LSTM backbone (backbones/lstm.py:4-48: nn.LSTM(2 -> H) with zero (h, c), fc_out H -> 2) with 33 .. 64 hidden units:
// the mapping of gru_wide.hip — ONE sequence per single-wave workgroup, LANE = HIDDEN UNIT — for four gates (nn.LSTM order i, f, g, o).
//   forward   the W_hh rows of gates i, f, g stay in the lane's registers (3 x 64), gate o's row is read from a padded LDS copy (row stride
//             65: lane = unit reads are conflict-free); the state is broadcast through LDS once per step; fc_out with lane = time step on
//             64-step chunks; i, f, g, o, c and h of every step go to the per-sequence record in HBM (`ckpt`: B x T x 6 x 64 floats) when a
//             backward pass follows;
//   backward  chunks in reverse; the lane of unit k forms dL/dh(t-1)[k] from the four gate gradients (broadcast through LDS) and column k
//             of W_hh (staged parameters: consecutive lanes, consecutive addresses); dW_hh as outer products on the 4-block MFMA with
//             the state rotated by 0 / 16 / 32 / 48 lanes (4 gates x 4 rotations x 16 accumulators = the whole AGPR file), dW_ih, the
//             biases and fc_out on the VALU.  One row of partial gradients per workgroup (every entry written).
// The state route (ODPD_FLAG_INIT_STATE, 1 .. 64 hidden units; lstm.py:46 passes (h_0, h_0)) runs the same bodies with S0 set: h and c both
// start at h0[b][unit], the backward takes h0 as h(-1) and c(-1), and writes dL/dh0 = dL/dh(-1) + dL/dc(-1) to dh0[b][unit].  The bodies are
// #included inside both kernels (lstm_wide_{fwd,bwd}_body.h), as in gru_wide.hip, so that the S0 = false kernels keep their instructions.
#include "odpd_seq.h"
#include "odpd_quant.h"

namespace odpd {
namespace {
constexpr int kLC = 64;          // time steps per chunk
constexpr int kLS = 65;          // row stride of the per-chunk [time][unit] arrays and of the padded gate-o rows
constexpr int kLHs = ((kLC + 1) * kLS + 3) & ~3;
constexpr int kLNS = 6;          // record of a step: i, f, g, o, c, h

__host__ __device__ inline int lstmw_fwd_floats(int P) { return pad4(P) + kLC * 2 + 64 + kLC * kLS + 64 * kLS; }
__host__ __device__ inline int lstmw_bwd_floats(int P) { return pad4(P) + kLC * 2 + kLC * 2 + kLC * 2 + 4 * 64 + kLHs; }

template <bool SAVE>
__global__ __launch_bounds__(64) void wide_lstm_fwd_kernel(SeqArgs a) {
    constexpr bool S0 = false;
#include "lstm_wide_fwd_body.h"
}
template <bool SAVE>
__global__ __launch_bounds__(64) void wide_lstm_fwd_state_kernel(SeqArgs a) {
    constexpr bool S0 = true;
#include "lstm_wide_fwd_body.h"
}

template <bool NW, bool DX>
__global__ __launch_bounds__(64) void wide_lstm_bwd_kernel(SeqArgs a) {
    constexpr bool S0 = false;
#include "lstm_wide_bwd_body.h"
}
template <bool NW, bool DX>
__global__ __launch_bounds__(64) void wide_lstm_bwd_state_kernel(SeqArgs a) {
    constexpr bool S0 = true;
#include "lstm_wide_bwd_body.h"
}

}  // namespace

// lstm of 33 .. 64 hidden units, float or with a quantised head (bits_w > 0: fc_out as INT_Linear; vdlstm's quantised heads keep the 32-unit envelope)
bool lstm_wide_ok(const odpd_model_t* m) {
    return m->backbone == ODPD_LSTM && m->hidden > 32 && m->hidden <= 64 && !(m->flags & ODPD_FLAG_TWO_LAYERS) &&
           (m->bits_w == 0 || (m->bits_w <= 16 && m->bits_a > 0 && m->bits_a <= 16));
}
int64_t lstm_wide_ckpt_floats(const odpd_model_t*, int B, int T) { return (int64_t)B * T * kLNS * 64; }
int lstm_wide_rows(const odpd_model_t*, int B) { const int cap = 4 * device_cus(); return B < cap ? B : cap; }
int lstm_wide_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!lstm_wide_ok(m)) return ODPD_EUNSUPPORTED;
    const size_t lds = (size_t)lstmw_fwd_floats(lstm_layout(m->hidden, 0, m->bits_w > 0).P) * sizeof(float);
    const int grid = lstm_wide_rows(m, a.B);
    return a.ckpt ? launch_seq(st, wide_lstm_fwd_kernel<true>, grid, lds, a) : launch_seq(st, wide_lstm_fwd_kernel<false>, grid, lds, a);
}
int lstm_wide_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!lstm_wide_ok(m)) return ODPD_EUNSUPPORTED;
    if (!a.ckpt) return ODPD_EINVAL;
    const size_t lds = (size_t)lstmw_bwd_floats(lstm_layout(m->hidden, 0, m->bits_w > 0).P) * sizeof(float);
    const int grid = lstm_wide_rows(m, a.B);
    const bool nw = a.partials != nullptr, dx = a.dx != nullptr;
    if (nw && dx) return launch_seq(st, wide_lstm_bwd_kernel<true, true>, grid, lds, a);
    if (nw) return launch_seq(st, wide_lstm_bwd_kernel<true, false>, grid, lds, a);
    return launch_seq(st, wide_lstm_bwd_kernel<false, true>, grid, lds, a);
}

// the state route: float lstm of 1 .. 64 hidden units, one layer, from a caller-given initial state (a.h0 = h(-1) = c(-1))
bool lstm_state_ok(const odpd_model_t* m) {
    return m->backbone == ODPD_LSTM && m->bits_w == 0 && m->hidden >= 1 && m->hidden <= 64 && !(m->flags & ODPD_FLAG_TWO_LAYERS);
}
int lstm_state_fwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!lstm_state_ok(m)) return ODPD_EUNSUPPORTED;
    if (!a.h0) return ODPD_EINVAL;
    const size_t lds = (size_t)lstmw_fwd_floats(lstm_layout(m->hidden, 0, false).P) * sizeof(float);
    const int grid = lstm_wide_rows(m, a.B);
    return a.ckpt ? launch_seq(st, wide_lstm_fwd_state_kernel<true>, grid, lds, a) : launch_seq(st, wide_lstm_fwd_state_kernel<false>, grid, lds, a);
}
int lstm_state_bwd(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) {
    if (!lstm_state_ok(m)) return ODPD_EUNSUPPORTED;
    if (!a.ckpt || !a.h0) return ODPD_EINVAL;
    const size_t lds = (size_t)lstmw_bwd_floats(lstm_layout(m->hidden, 0, false).P) * sizeof(float);
    const int grid = lstm_wide_rows(m, a.B);
    const bool nw = a.partials != nullptr, dx = a.dx != nullptr;      // (neither: dL/dh0 alone)
    if (nw && dx) return launch_seq(st, wide_lstm_bwd_state_kernel<true, true>, grid, lds, a);
    if (nw) return launch_seq(st, wide_lstm_bwd_state_kernel<true, false>, grid, lds, a);
    if (dx) return launch_seq(st, wide_lstm_bwd_state_kernel<false, true>, grid, lds, a);
    return launch_seq(st, wide_lstm_bwd_state_kernel<false, false>, grid, lds, a);
}

}  // namespace odpd
