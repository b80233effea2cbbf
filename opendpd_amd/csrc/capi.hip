// capi.hip — the extern "C" surface declared in include/opendpd_hip.h: argument validation and
// dispatch to the backbone families.
#include <dlfcn.h>

#include <mutex>
#include <set>
#include <utility>

#include "odpd_host.h"
#include "odpd_xchg.h"

using namespace odpd;

namespace {
enum Family { FAM_NONE = 0, FAM_GRU, FAM_LSTM, FAM_DELTA, FAM_JANET, FAM_TCNN, FAM_QAT, FAM_GMP, FAM_RVTDCNN, FAM_DVR, FAM_BOJ, FAM_APN, FAM_MCL, FAM_GRU2, FAM_QCELL };
inline Family family_of(int bb);
// a quantisation-aware model: bits_w > 0 on one of the backbones the reference's surgery turns into a quantised cell
// (quant/quant_envs.py:114-130, 290-306: gru, dgru, qgru, qgru_amp1 through the GRU swap; deltagru_tcnskip through its op modules)
inline Family family_of(const odpd_model_t* m) {
    // ODPD_FLAG_QUANT_CELL, ODPD_FLAG_TWO_LAYERS: families of their own, so that whatever is written for a backbone's one-layer float kernels
    // (`family_of(m) == FAM_...`: f4_of, fused_step, the cascade) finds none for these descriptors instead of misreading their parameter buffer;
    // their kernels are kRoutes' (route_of)
    if (m->flags & ODPD_FLAG_QUANT_CELL) return FAM_QCELL;
    if (m->flags & ODPD_FLAG_TWO_LAYERS) return FAM_GRU2;
    if (m->bits_w > 0 && (m->backbone == ODPD_QGRU || m->backbone == ODPD_QGRU_AMP1 || m->backbone == ODPD_GRU || m->backbone == ODPD_DGRU ||
                          m->backbone == ODPD_TRES_DELTAGRU))
        return FAM_QAT;
    return family_of((int)m->backbone);
}
inline Family family_of(int bb) {
    switch (bb) {
    case ODPD_GRU: case ODPD_DGRU: case ODPD_QGRU: case ODPD_QGRU_AMP1: return FAM_GRU;
    case ODPD_LSTM: case ODPD_VDLSTM: return FAM_LSTM;
    case ODPD_DELTAGRU: case ODPD_TRES_DELTAGRU: case ODPD_DELTAJANET: return FAM_DELTA;
    case ODPD_PGJANET: return FAM_JANET;
    case ODPD_TCNN: case ODPD_NEURALTX: return FAM_TCNN;
    case ODPD_GMP: return FAM_GMP;
    case ODPD_RVTDCNN: return FAM_RVTDCNN;
    case ODPD_DVRJANET: return FAM_DVR;
    case ODPD_BOJANET: return FAM_BOJ;
    case ODPD_APNRRU: return FAM_APN;
    case ODPD_MCLDNN: return FAM_MCL;
    default: return FAM_NONE;
    }
}
inline int feat_dim(int bb) {
    switch (bb) {
    case ODPD_GRU: case ODPD_LSTM: return 2;
    case ODPD_DGRU: case ODPD_DELTAGRU: case ODPD_TRES_DELTAGRU: case ODPD_DELTAJANET: case ODPD_TCNN: return 6;
    case ODPD_QGRU: case ODPD_QGRU_AMP1: case ODPD_VDLSTM: return 4;
    default: return 0;
    }
}
inline bool init_state(const odpd_model_t* m) { return (m->flags & ODPD_FLAG_INIT_STATE) != 0; }
inline bool quant_cell(const odpd_model_t* m) { return (m->flags & ODPD_FLAG_QUANT_CELL) != 0; }

// ---- table 1: the kernel sets that are forward / backward only.  The fused entry points answer ODPD_EUNSUPPORTED for their descriptors and
// the caller chains forward, loss, backward ----
using SeqFn = int (*)(hipStream_t, const odpd_model_t*, const SeqArgs&);
struct Route {
    bool (*ok)(const odpd_model_t*);
    int64_t (*param_count)(const odpd_model_t*);      // NULL: the backbone's formula in odpd_param_count
    int64_t (*ckpt_floats)(const odpd_model_t*, int B, int T);
    int (*rows)(const odpd_model_t*, int B);
    SeqFn fwd, bwd;
};
constexpr Route kRoutes[] = {
    // ODPD_FLAG_INIT_STATE, a caller-given initial state: the lane-per-unit kernels of gru_wide.hip / lstm_wide.hip (their per-step records and
    // rows) at every hidden size 1 .. 64, one layer, float; launched by odpd_backbone_fwd_state / _bwd_state alone
    {gru_state_ok, nullptr, gru_wide_ckpt_floats, gru_wide_rows, gru_state_fwd, gru_state_bwd},
    {lstm_state_ok, nullptr, lstm_wide_ckpt_floats, lstm_wide_rows, lstm_state_fwd, lstm_state_bwd},
    // ODPD_FLAG_QUANT_CELL, `--quant` inside the cell: eight INT_Linear on bojanet, nine on dvrjanet, 1 .. 16 hidden units
    {bojanet_q_ok, bojanet_q_param_count, bojanet_q_ckpt_floats, bojanet_q_rows, bojanet_q_fwd, bojanet_q_bwd},
    {dvrjanet_q_ok, dvrjanet_q_param_count, dvrjanet_q_ckpt_floats, dvrjanet_q_rows, dvrjanet_q_fwd, dvrjanet_q_bwd},
    // ODPD_FLAG_TWO_LAYERS: two recurrent layers in one wave, 1 .. 32 hidden units
    {gru2_ok, gru2_param_count, gru2_ckpt_floats, gru2_rows, gru2_fwd, gru2_bwd},
    {lstm2_ok, lstm2_param_count, lstm2_ckpt_floats, lstm2_rows, lstm2_fwd, lstm2_bwd},
    // by hidden size: lane per unit at 33 .. 64 (pgjanet: 17 .. 32; deltajanet with quantised heads: every size), and the pgjanet of six INT_Linear
    {gru_wide_ok, nullptr, gru_wide_ckpt_floats, gru_wide_rows, gru_wide_fwd, gru_wide_bwd},
    {lstm_wide_ok, nullptr, lstm_wide_ckpt_floats, lstm_wide_rows, lstm_wide_fwd, lstm_wide_bwd},
    {vdlstm_wide_ok, nullptr, vdlstm_wide_ckpt_floats, vdlstm_wide_rows, vdlstm_wide_fwd, vdlstm_wide_bwd},
    {delta_wide_ok, nullptr, delta_wide_ckpt_floats, delta_wide_rows, delta_wide_fwd, delta_wide_bwd},
    {deltajanet_wide_ok, nullptr, deltajanet_wide_ckpt_floats, deltajanet_wide_rows, deltajanet_wide_fwd, deltajanet_wide_bwd},
    {pgjanet_wide_ok, nullptr, pgjanet_wide_ckpt_floats, pgjanet_wide_rows, pgjanet_wide_fwd, pgjanet_wide_bwd},
    {pgjanet_q_ok, pgjanet_q_param_count, pgjanet_q_ckpt_floats, pgjanet_q_rows, pgjanet_q_fwd, pgjanet_q_bwd},
};
enum { ROUTE_NONE = -1, ROUTE_REFUSED = -2, kStateRoutes = 0, kQuantCellRoutes = 2, kTwoLayerRoutes = 4, kHiddenRoutes = 6, kNumRoutes = 13 };
static_assert(sizeof(kRoutes) / sizeof(kRoutes[0]) == kNumRoutes, "kRoutes and its group bounds");
// Which of kRoutes serves a descriptor: its index; ROUTE_NONE — not a descriptor of these routes (the family kernels below answer for it);
// ROUTE_REFUSED — it asks for such a route and none serves it: every entry point answers ODPD_EUNSUPPORTED.
// A flag selects its group alone, in this order: ODPD_FLAG_INIT_STATE first (with ODPD_FLAG_QUANT_CELL on top: refused), then
// ODPD_FLAG_QUANT_CELL, then ODPD_FLAG_TWO_LAYERS, then the routes chosen by hidden size — so no flag is ever answered by a kernel that
// would misread the flagged model's parameter buffer.  Without a flag only a pgjanet with bits_w > 0 that the table's last row does not take is refused.
inline int route_of(const odpd_model_t* m) {
    const auto first = [m](int lo, int hi, int miss) {
        for (int k = lo; k < hi; ++k)
            if (kRoutes[k].ok(m)) return k;
        return miss;
    };
    if (init_state(m)) return quant_cell(m) ? (int)ROUTE_REFUSED : first(kStateRoutes, kQuantCellRoutes, ROUTE_REFUSED);
    if (quant_cell(m)) return first(kQuantCellRoutes, kTwoLayerRoutes, ROUTE_REFUSED);
    if (m->flags & ODPD_FLAG_TWO_LAYERS) return first(kTwoLayerRoutes, kHiddenRoutes, ROUTE_REFUSED);
    return first(kHiddenRoutes, kNumRoutes, m->backbone == ODPD_PGJANET && m->bits_w > 0 ? ROUTE_REFUSED : ROUTE_NONE);
}
// the float GRU family on its own kernels (gru_family.hip, gru_s16*.hip): what the frozen-PA loss step and the sweeps serve
inline bool gru_family_model(const odpd_model_t* m) { return family_of(m) == FAM_GRU && route_of(m) == ROUTE_NONE; }
// bits_w > 0 selects a quantised model only where one exists (include/opendpd_hip.h, odpd_model_t::bits_w); on every other backbone
// the descriptor is refused outright — no entry point may answer it with the float kernels on a float parameter layout
inline bool quant_desc_ok(const odpd_model_t* m) {
    if (m->bits_w <= 0 || m->backbone == ODPD_DVRJANET) return true;      // (dvrjanet: bits_w carries num_dvr_units)
    if (quant_cell(m)) return true;      // (what the flag is valid on is answered with ODPD_EUNSUPPORTED, not here: route_of)
    switch (m->backbone) {
    case ODPD_GRU: case ODPD_DGRU: case ODPD_QGRU: case ODPD_QGRU_AMP1: case ODPD_TRES_DELTAGRU:      // the surgery's quantised cells
    case ODPD_LSTM: case ODPD_VDLSTM: case ODPD_DELTAJANET: case ODPD_NEURALTX:                      // float core, INT_Linear heads
    case ODPD_RVTDCNN:                                                                               // INT_Conv2D + INT_Linear layers (rvtdcnn_q.hip)
    case ODPD_PGJANET:                                                                               // six INT_Linear (pgjanet_q.hip)
        return m->bits_a > 0;
    default: return false;
    }
}
inline bool model_ok(const odpd_model_t* m) {
    return m && m->backbone >= 0 && m->backbone < ODPD_BACKBONE_COUNT && m->hidden > 0 && quant_desc_ok(m);
}
inline SeqArgs make_args(const odpd_model_t* m, int B, int T) {
    SeqArgs a{};
    a.B = B; a.T = T; a.H = m->hidden;
    a.ngroups = num_groups(B, rows_per_seq(m->hidden) ? rows_per_seq(m->hidden) : 1);
    a.nck = num_ckpt(T);
    a.thx = m->thx; a.thh = m->thh;
    a.bits_w = m->bits_w; a.bits_a = m->bits_a; a.eval_out = (m->flags & ODPD_FLAG_EVAL) ? 1 : 0;
    return a;
}

// ---- table 2: dvrjanet, bojanet, apnrru and mcldnn on the 16-sequences-per-wave f4 mapping share one interface ----
template <int (*LAUNCH)(hipStream_t, const odpd_model_t*, const SeqArgs&, int), int MODE>      // (mode 1 forward, 2 backward)
int f4_call(hipStream_t st, const odpd_model_t* m, const SeqArgs& a) { return LAUNCH(st, m, a, MODE); }
struct F4Backbone {
    SeqFn fwd, bwd;
    int (*rows)(const odpd_model_t*, int B);
    int64_t (*param_count)(const odpd_model_t*);
    int64_t (*ckpt_floats)(const odpd_model_t*, int B, int T);
    bool (*train_uses_gp)(const odpd_model_t*, int B, int T);      // the gate-parallel fused train kernel takes the shape (the reference's batch sizes)
    int (*gp_rows)(const odpd_model_t*, int B, int T);
    SeqFn gp_train;
};
constexpr F4Backbone kF4[] = {      // FAM_DVR .. FAM_MCL, in the enum's order
    // K + 7H^2 + 7H + 2 parameters, K = bits_w (dvrjanet.py:11-30, 47-52)
    {f4_call<dvrjanet_launch, 1>, f4_call<dvrjanet_launch, 2>, dvrjanet_rows, dvrjanet_param_count, dvrjanet_ckpt_floats, dvrjanet_train_uses_gp, dvrjanet_gp_rows, dvrjanet_gp_train},
    // 2H^2 + 28H + 194 (bojanet.py:15-26)
    {f4_call<bojanet_launch, 1>, f4_call<bojanet_launch, 2>, bojanet_rows, bojanet_param_count, bojanet_ckpt_floats, bojanet_train_uses_gp, bojanet_gp_rows, bojanet_gp_train},
    // 343 + 70H (apnrru.py:13-19, 45-53)
    {f4_call<apnrru_launch, 1>, f4_call<apnrru_launch, 2>, apnrru_rows, apnrru_param_count, apnrru_ckpt_floats, apnrru_train_uses_gp, apnrru_gp_rows, apnrru_gp_train},
    // 190C + 589 (mcldnn.py:21-27)
    {f4_call<mcldnn_launch, 1>, f4_call<mcldnn_launch, 2>, mcldnn_rows, mcldnn_param_count, mcldnn_ckpt_floats, mcldnn_train_uses_gp, mcldnn_gp_rows, mcldnn_gp_train},
};
static_assert(FAM_BOJ == FAM_DVR + 1 && FAM_APN == FAM_DVR + 2 && FAM_MCL == FAM_DVR + 3, "kF4 is indexed by family");
inline const F4Backbone* f4_of(const odpd_model_t* m) {      // (family_of: a flagged descriptor is none of them)
    const Family f = family_of(m);
    return f >= FAM_DVR && f <= FAM_MCL ? &kF4[f - FAM_DVR] : nullptr;
}

// ---- the fused train step (forward + loss + backward in one launch), resolved once per (m, B, T) ----
// what the `workspace` pointer of odpd_train_fwd_bwd / odpd_train_fwd_bwd_framed is to the kernel: nothing; BPTT checkpoints (ws_floats of them);
// the four sparsity counters of the step's forward pass (double[4], may be NULL — delta backbones and the quantised TRes-DeltaGRU)
enum WsKind { WS_UNUSED, WS_CKPT, WS_COUNTERS };
struct FusedStep {
    SeqFn train;            // NULL: the family has no fused kernel for this shape
    int64_t rows;           // partial-gradient rows the launch writes (odpd_partial_rows(fused = 1))
    int64_t ws_floats;      // floats behind `workspace` (odpd_train_workspace_floats)
    WsKind ws;
    bool framed;            // the kernel addresses frames inside resident streams (SeqArgs::frame_idx): the framed entry points serve the shape
};
inline FusedStep fused_step(const odpd_model_t* m, int B, int T) {
    const FusedStep none{nullptr, ODPD_EUNSUPPORTED, ODPD_EUNSUPPORTED, WS_UNUSED, false};
    const int r = route_of(m);
    // (kept as it was before the table: a pgjanet whose bit widths no kernel takes is ROUTE_REFUSED, yet of the fused entry points only
    // odpd_partial_rows ever asked; the others serve its hidden <= 16 as the float model)
    const bool float_pgjanet = r == ROUTE_REFUSED && family_of(m) == FAM_JANET && !init_state(m);
    if (r != ROUTE_NONE && !float_pgjanet) return none;
    if (const F4Backbone* f = f4_of(m)) return f->train_uses_gp(m, B, T) ? FusedStep{f->gp_train, f->gp_rows(m, B, T), 0, WS_UNUSED, true} : none;
    const auto ws_of = [](KernelSet fused) { return fused == KS_S16 || fused == KS_S16N || fused == KS_S16X ? WS_CKPT : WS_UNUSED; };
    switch (family_of(m)) {
    case FAM_GRU: {    // every shape, from tensors and from frames (a model the family does not take: the launcher and the rows refuse, each for itself)
        const GruPlan p = gru_plan(m, B, T, GRU_PLAN_FUSED);
        return {gru_family_train, p.fused_rows, p.ws_floats, ws_of(p.fused), true};
    }
    case FAM_LSTM: {   // (the 16-sequences-per-wave kernel takes tensors only)
        const SplitPlan p = lstm_plan(m, B, T);
        if (p.fused == KS_NONE) return none;
        return {p.fused == KS_S16 ? lstm_s16_train : lstm_gp_train, p.fused_rows, p.ws_floats, ws_of(p.fused), p.fused != KS_S16};
    }
    case FAM_JANET: {
        const SplitPlan p = janet_plan(m, B, T);
        return p.fused == KS_NONE ? none : FusedStep{janet_gp_train, p.fused_rows, p.ws_floats, WS_UNUSED, true};
    }
    case FAM_DELTA: {  // (the launcher is named at every shape: odpd_train_fwd_bwd calls it without asking and lets it answer; sizes and frames ask)
        const SplitPlan p = delta_plan(m, B, T);
        return {delta_gp_train, p.fused_rows, p.ws_floats, WS_COUNTERS, p.fused != KS_NONE};
    }
    // (the launchers answer for a hidden size they do not take; the workspace query refuses it in front of them)
    case FAM_GMP: return {gmp_train, gmp_rows(m, B, T), odpd_param_count(m) > 0 ? 0 : (int64_t)ODPD_EUNSUPPORTED, WS_UNUSED, true};
    case FAM_RVTDCNN: return {rvtdcnn_train, rvtdcnn_train_rows(m, B, T), odpd_param_count(m) > 0 ? 0 : (int64_t)ODPD_EUNSUPPORTED, WS_UNUSED, true};
    case FAM_QAT: {
        const SplitPlan p = qat_plan(m, B, T);
        if (p.fused == KS_NONE) return none;
        return {qat_family_train, p.fused_rows, p.ws_floats, p.fused == KS_S16 ? WS_CKPT : m->backbone == ODPD_TRES_DELTAGRU ? WS_COUNTERS : WS_UNUSED, true};
    }
    default: return none;
    }
}

// ---- the split calls (forward, backward from dL/dy) and their two buffers, resolved once per (m, B, T) ----
struct SplitStep {
    SeqFn fwd, bwd;           // NULL: no kernel serves the descriptor (ODPD_EUNSUPPORTED)
    int64_t ckpt_floats;      // odpd_ckpt_floats
    int64_t rows;             // odpd_partial_rows(fused = 0)
    bool need_ckpt;           // a backward without checkpoints over more than one block is ODPD_EINVAL (the row-rotated kernels restart every block but the first from one)
};
inline SplitStep split_step(const odpd_model_t* m, int B, int T) {
    const SplitStep none{nullptr, nullptr, ODPD_EUNSUPPORTED, ODPD_EUNSUPPORTED, false};
    const int r = route_of(m);
    if (r == ROUTE_REFUSED) return none;
    if (r >= 0) return {kRoutes[r].fwd, kRoutes[r].bwd, kRoutes[r].ckpt_floats(m, B, T), kRoutes[r].rows(m, B), false};
    if (const F4Backbone* f = f4_of(m)) return {f->fwd, f->bwd, f->ckpt_floats(m, B, T), f->rows(m, B), false};
    const auto of = [](SeqFn fwd, SeqFn bwd, const SplitPlan& p) { return SplitStep{fwd, bwd, p.ckpt_floats, p.bwd_rows, p.need_ckpt}; };
    switch (family_of(m)) {
    case FAM_GRU: return of(gru_family_fwd, gru_family_bwd, gru_plan(m, B, T, GRU_PLAN_SPLIT));
    case FAM_LSTM: return of(lstm_family_fwd, lstm_family_bwd, lstm_plan(m, B, T));
    case FAM_DELTA: return of(delta_family_fwd, delta_family_bwd, delta_plan(m, B, T));
    case FAM_JANET: return of(janet_family_fwd, janet_family_bwd, janet_plan(m, B, T));
    case FAM_QAT: return of(qat_family_fwd, qat_family_bwd, qat_plan(m, B, T));
    case FAM_TCNN: return {tcnn_fwd, tcnn_bwd, 0, tcnn_rows(m, B, T), false};      // (these three are not recurrent: nothing to checkpoint)
    case FAM_GMP: return {gmp_fwd, gmp_bwd, 0, gmp_rows(m, B, T), false};
    case FAM_RVTDCNN: return {rvtdcnn_fwd, rvtdcnn_bwd, 0, rvtdcnn_rows(m, B, T), false};
    default: return none;
    }
}
}  // namespace

#include <stdlib.h>
#include <string.h>
#include <vector>
odpd::Tuning& odpd::tuning() {
    static Tuning t = [] {
        Tuning v;
        const char* e = getenv("ODPD_S16_MIN_BATCH");
        v.s16_min_batch = e ? atol(e) : -1;   // -1 = built-in crossover
        e = getenv("ODPD_S16_OCCUPANCY");
        v.s16_occupancy = e ? atoi(e) : 0;    // 0 = by batch size
        e = getenv("ODPD_GP_MAX_BATCH");
        v.gp_max_batch = e ? atol(e) : -1;    // -1 = built-in crossover, 0 = never the gate-parallel fused train kernel
        e = getenv("ODPD_CASCADE_ONE_LAUNCH");
        v.cascade_one_launch = e ? atoi(e) : 1;   // 0 = train_dpd steps always as chained launches
        e = getenv("ODPD_XCHG_FUSED");
        v.xchg_fused = e ? atoi(e) : 1;           // 0 = the one-shot exchange as its own launch instead of the optimiser kernel's prologue
        e = getenv("ODPD_S16X");
        v.s16x = e ? atoi(e) : 1;                 // 0 = frozen-PA step of hidden 17 .. 24 on the exact-fp32 kernel (gru_s16n.hip) instead of the bf16x3 one
        e = getenv("ODPD_S16X_TRAIN");
        v.s16x_train = e ? atoi(e) : 1;           // 0 = fused train step of hidden 17 .. 24 on the exact-fp32 kernel (gru_s16n.hip) instead of the bf16x3 one
        e = getenv("ODPD_LSTM_PACK");
        v.lstm_pack = e ? atoi(e) : 1;            // 0 = lstm16_train_kernel without K-packed input slots (hidden <= 13)
        e = getenv("ODPD_QAT_U3");
        v.qat_u3 = e ? atoi(e) : 1;               // 0 = quantisation-aware GRUCell kinds of hidden <= 12 with four unit slots per lane instead of three (qat_s16.hip)
        return v;
    }();
    return t;
}
// ODPD_AUDIT_LDS (odpd_seq.h): one stderr line per distinct (kernel, dynamic LDS bytes)
void odpd::audit_lds(const void* kernel, size_t lds) {
    static const bool on = getenv("ODPD_AUDIT_LDS") != nullptr;
    if (!on) return;
    static std::mutex mu;
    static std::set<std::pair<const void*, size_t>> seen;
    std::lock_guard<std::mutex> lock(mu);
    if (!seen.insert({kernel, lds}).second) return;
    Dl_info info;
    hipFuncAttributes at;
    const bool named = dladdr(kernel, &info) != 0 && info.dli_sname != nullptr;
    const int regs = hipFuncGetAttributes(&at, kernel) == hipSuccess ? at.numRegs : -1;
    fprintf(stderr, "[odpd-lds] %s lds=%zu regs=%d\n", named ? info.dli_sname : "?", lds, regs);
}
static int64_t g_tuning_generation = 0;
extern "C" int odpd_set_tuning(const char* key, int64_t value) {
    if (!key) return ODPD_EINVAL;
    if (!strcmp(key, "s16_min_batch")) { tuning().s16_min_batch = (long)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "s16_occupancy")) { tuning().s16_occupancy = (int)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "gp_max_batch")) { tuning().gp_max_batch = (long)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "cascade_one_launch")) { tuning().cascade_one_launch = (int)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "xchg_fused")) { tuning().xchg_fused = (int)value; return 0; }      // (no buffer depends on it)
    if (!strcmp(key, "s16x")) { tuning().s16x = (int)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "s16x_train")) { tuning().s16x_train = (int)value; ++g_tuning_generation; return 0; }
    if (!strcmp(key, "lstm_pack")) { tuning().lstm_pack = (int)value; return 0; }      // (same buffers either way)
    if (!strcmp(key, "qat_u3")) { tuning().qat_u3 = (int)value; ++g_tuning_generation; return 0; }   // (same buffer sizes, but the slot count maps units into each checkpoint record)
    return ODPD_EINVAL;
}
extern "C" int64_t odpd_tuning_generation(void) { return g_tuning_generation; }

// ---- odpd_probe_issue_ns: vector-issue speed of this GPU ---------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_issue_kernel(float* out, int iters, float b, float c) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (float)(threadIdx.x + j) * 1e-6f;
    const float x = (float)threadIdx.x * c;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = __builtin_fmaf(x, b, a[j]);          // 8 independent accumulate chains x 8 = 64 v_fmac_f32
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a[j];
    if (s == 123.456f) out[blockIdx.x * blockDim.x + threadIdx.x] = s;              // (keeps the chains alive; never true for these operands)
}
extern "C" int odpd_probe_issue_ns(void* stream, int iters, double* ns_per_wave_instr) {
    if (iters < 1 || ns_per_wave_instr == nullptr) return ODPD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* out = nullptr;
    const int blocks = device_cus() * 4;             // 4 workgroups of 4 waves per CU = four waves per SIMD
    if (hipMalloc(&out, (size_t)blocks * 256 * sizeof(float)) != hipSuccess) return ODPD_EINVAL;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 0.0f;
    for (int pass = 0; pass < 2; ++pass) {
        hipEventRecord(e0, st);
        hipLaunchKernelGGL(probe_issue_kernel, dim3(blocks), dim3(256), 0, st, out, iters, 0.999f, 1e-3f);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(out);
    *ns_per_wave_instr = (double)ms * 1e6 / ((double)iters * 64.0 * 4.0);
    return (int)hipGetLastError();
}

extern "C" int odpd_abi_version(void) { return 13; }   // 13: + odpd_probe_issue_ns; + ODPD_FLAG_INIT_STATE, odpd_backbone_fwd_state / _bwd_state (backward compatible: no existing call changes); 12: + odpd_sweep_* / odpd_train_epoch_sweep / odpd_backbone_fwd_sweep (K runs of one model shape in lockstep: one launch per step carries them all); 11: + ODPD_FLAG_TWO_LAYERS (gru / qgru / qgru_amp1 with two recurrent layers), hidden 33 .. 64 for the GRU family and lstm, bits_w > 0 on lstm / vdlstm (INT_Linear heads); 10: + odpd_xchg_* (one-shot gradient exchange over peer-mapped slots), odpd_clip_optim_step_dp, odpd_comm_kind / _errors; 9: + odpd_cascade_rows, odpd_cascade_fwd_bwd (train_dpd step body in one launch); 8: + odpd_comm_*, odpd_shard_range, odpd_train_epoch_dp (RCCL inside the native step path); 7: quantised gru / dgru / deltagru_tcnskip descriptors (bits_w > 0), QAT hidden <= 32; 3: + odpd_clip_adamw_step_masked, odpd_tuning_generation, backbones 11..13; 4: backbones 14..17; 5: + odpd_framed_train_supported_shape; 6: + odpd_train_epoch_split
extern "C" const char* odpd_built_arch(void) { return "gfx950"; }

extern "C" int64_t odpd_param_count(const odpd_model_t* m) {
    if (!model_ok(m)) return ODPD_EINVAL;
    const int r = route_of(m);
    if (r == ROUTE_REFUSED) return ODPD_EUNSUPPORTED;
    if (r >= 0 && kRoutes[r].param_count) return kRoutes[r].param_count(m);
    if (family_of(m) == FAM_QAT) return qat_s16_param_count(m);
    if (const F4Backbone* f = f4_of(m)) return f->param_count(m);
    const int64_t H = m->hidden, F = feat_dim(m->backbone);
    switch (m->backbone) {
    case ODPD_GRU: case ODPD_QGRU: case ODPD_QGRU_AMP1: return 3 * H * F + 3 * H * H + 6 * H + 2 * H + 2;
    case ODPD_DGRU: return 3 * H * F + 3 * H * H + 6 * H + 2 * (H + 6) + 2 + H * H + H;
    // bits_w > 0 on lstm / vdlstm: their nn.Linear heads are INT_Linear (+ three scale parameters each; quant_envs.py:40-60)
    case ODPD_LSTM: return 4 * H * F + 4 * H * H + 8 * H + 2 * H + 2 + (m->bits_w > 0 ? 3 : 0);
    case ODPD_VDLSTM: return 4 * H * 4 + 4 * H * H + 8 * H + 2 * (4 * H + 4) + 2 * 8 + 2 + (m->bits_w > 0 ? 9 : 0);
    case ODPD_DELTAGRU: return 3 * H * 6 + 3 * H * H + 6 * H + 2 * H + 2;
    case ODPD_TRES_DELTAGRU: return 3 * H * 6 + 3 * H * H + 2 * H + 18 + 6;
    case ODPD_DELTAJANET: return 2 * H * 6 + 2 * H * H + 4 * H + 2 * H + 2 + (m->bits_w > 0 ? 3 : 0);      // two gates (deltajanet.py:96-111) + fc_out (bits_w > 0: INT_Linear, + three scales)
    case ODPD_TCNN: return 6 * H + H + 4 * 5 * H + 2 * H;
    case ODPD_PGJANET: return 3 * (H * (H + 1) + H) + 2 * (H * 2 * H + H) + 2 * H + 2;      // (bits_w > 0: kRoutes)
    case ODPD_NEURALTX: return H <= 64 ? 27 * H + 14 + (m->bits_w > 0 ? 3 : 0) : (int64_t)ODPD_EUNSUPPORTED;   // two 5-tap FIRs, 4->C (+bias), 4 x depthwise k5, C->2, IQ_match 2x2 (bits_w > 0: INT_Linear, + three scales)
    case ODPD_GMP: return H == 11 ? H * (1 + 4 * H) : (int64_t)ODPD_EUNSUPPORTED;   // memory_length 11, degree 5 (models.py:26-28)
    case ODPD_RVTDCNN: return H <= 32 ? (m->bits_w > 0 ? rvtdcnn_q_param_count(m) : 39 * H + 32) : (int64_t)ODPD_EUNSUPPORTED;  // conv 27+3, fc_hid 36H+H, fc_out 2H+2 (rvtdcnn.py:19-33)
    default: return ODPD_EUNSUPPORTED;
    }
}

extern "C" int64_t odpd_ckpt_floats(const odpd_model_t* m, int B, int T) {
    if (!model_ok(m) || B <= 0 || T <= 0) return ODPD_EINVAL;
    return split_step(m, B, T).ckpt_floats;
}

extern "C" int64_t odpd_partial_rows(const odpd_model_t* m, int B, int T, int fused) {
    if (!model_ok(m) || B <= 0 || T <= 0) return ODPD_EINVAL;
    if (!fused) return split_step(m, B, T).rows;
    if (route_of(m) != ROUTE_NONE) return ODPD_EUNSUPPORTED;      // (forward / backward only: no fused rows)
    const FusedStep f = fused_step(m, B, T);
    return f.train ? f.rows : (int64_t)ODPD_EUNSUPPORTED;
}

extern "C" int64_t odpd_train_workspace_floats(const odpd_model_t* m, int B, int T) {
    if (!model_ok(m) || B <= 0 || T <= 0) return ODPD_EINVAL;
    const FusedStep f = fused_step(m, B, T);
    return f.train ? f.ws_floats : (int64_t)ODPD_EUNSUPPORTED;
}

extern "C" int odpd_backbone_fwd(void* stream, const odpd_model_t* m, int B, int T, const float* params,
                                 const float* x, float* y, float* ckpt, double* stats) {
    if (!model_ok(m) || !params || !x || !y || B <= 0 || T <= 0) return ODPD_EINVAL;
    const SplitStep s = split_step(m, B, T);
    if (!s.fwd) return ODPD_EUNSUPPORTED;
    if (init_state(m)) return ODPD_EINVAL;      // (served, but by odpd_backbone_fwd_state: this call has no h0)
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = x; a.y = y; a.ckpt = ckpt; a.stats = stats;
    return s.fwd((hipStream_t)stream, m, a);
}

extern "C" int odpd_backbone_bwd(void* stream, const odpd_model_t* m, int B, int T, const float* params,
                                 const float* x, const float* dy, const float* ckpt, float* partials, float* dx) {
    if (!model_ok(m) || !params || !x || !dy || B <= 0 || T <= 0 || (!partials && !dx)) return ODPD_EINVAL;
    const SplitStep s = split_step(m, B, T);
    if (!s.bwd) return ODPD_EUNSUPPORTED;
    if (init_state(m)) return ODPD_EINVAL;      // (served, but by odpd_backbone_bwd_state)
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = x; a.dy = dy; a.ckpt = const_cast<float*>(ckpt); a.partials = partials; a.dx = dx;
    if (s.need_ckpt && !ckpt && a.nck > 1) return ODPD_EINVAL;
    return s.bwd((hipStream_t)stream, m, a);
}

// the state route (ODPD_FLAG_INIT_STATE: route_of answers nothing but one of its two kernel sets, or ROUTE_REFUSED)
extern "C" int odpd_backbone_fwd_state(void* stream, const odpd_model_t* m, int B, int T, const float* params, const float* x, const float* h0,
                                       float* y, float* ckpt) {
    if (!model_ok(m) || !params || !x || !h0 || !y || B <= 0 || T <= 0 || !init_state(m)) return ODPD_EINVAL;
    const SplitStep s = split_step(m, B, T);
    if (!s.fwd) return ODPD_EUNSUPPORTED;
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = x; a.y = y; a.ckpt = ckpt; a.h0 = h0;
    return s.fwd((hipStream_t)stream, m, a);
}
extern "C" int odpd_backbone_bwd_state(void* stream, const odpd_model_t* m, int B, int T, const float* params, const float* x, const float* h0,
                                       const float* dy, const float* ckpt, float* partials, float* dx, float* dh0) {
    if (!model_ok(m) || !params || !x || !h0 || !dy || !ckpt || B <= 0 || T <= 0 || (!partials && !dx && !dh0) || !init_state(m))
        return ODPD_EINVAL;
    const SplitStep s = split_step(m, B, T);
    if (!s.bwd) return ODPD_EUNSUPPORTED;
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = x; a.dy = dy; a.ckpt = const_cast<float*>(ckpt); a.partials = partials; a.dx = dx; a.h0 = h0; a.dh0 = dh0;
    return s.bwd((hipStream_t)stream, m, a);
}

// `workspace` of the two fused entry points into the launch arguments, as the step's kernel takes it (WsKind)
static void set_workspace(SeqArgs& a, const FusedStep& f, float* workspace) {
    a.ckpt = workspace;      // (WS_UNUSED: handed on all the same, as it always was)
    if (f.ws == WS_COUNTERS) { a.stats = reinterpret_cast<double*>(workspace); a.ckpt = nullptr; }
}
extern "C" int odpd_train_fwd_bwd(void* stream, const odpd_model_t* m, int loss_kind, int B, int T, int64_t count,
                                  const float* params, const float* x, const float* target, float* partials,
                                  float* workspace) {
    if (!model_ok(m) || !params || !x || !target || !partials || B <= 0 || T <= 0 || count <= 0) return ODPD_EINVAL;
    const FusedStep f = fused_step(m, B, T);
    if (!f.train) return ODPD_EUNSUPPORTED;
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = x; a.target = target; a.partials = partials;
    a.inv_count = (float)(1.0 / (double)count); a.loss_kind = loss_kind;
    set_workspace(a, f, workspace);
    return f.train((hipStream_t)stream, m, a);      // (whatever f.rows says: a launcher named for a shape it does not take answers for itself)
}

// Frozen model in front of the loss (the PA of train_dpd): forward + loss + dL/du in ONE launch.  Available for the GRU family
// (row-rotated kernels with LDS-resident BPTT state at small batches, S16 / S16N at large ones); everywhere else
// ODPD_EUNSUPPORTED (rows < 0) and the caller chains odpd_backbone_fwd, odpd_loss_fwd_bwd, odpd_backbone_bwd.
extern "C" int64_t odpd_frozen_loss_rows(const odpd_model_t* m, int B, int T) {
    if (!model_ok(m) || B <= 0 || T <= 0) return ODPD_EINVAL;
    if (!gru_family_model(m)) return ODPD_EUNSUPPORTED;
    return gru_plan(m, B, T, GRU_PLAN_LOSSDX).loss_rows;
}
extern "C" int odpd_frozen_loss_dx(void* stream, const odpd_model_t* m, int loss_kind, int B, int T, int64_t count,
                                   const float* params, const float* u, const float* target, float* du, float* loss_rows,
                                   float* workspace) {
    if (!model_ok(m) || !params || !u || !target || !du || !loss_rows || !workspace || B <= 0 || T <= 0 || count <= 0) return ODPD_EINVAL;
    if (!gru_family_model(m)) return ODPD_EUNSUPPORTED;
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = u; a.target = target; a.dx = du; a.partials = loss_rows;
    a.inv_count = (float)(1.0 / (double)count); a.loss_kind = loss_kind; a.ckpt = workspace;
    return gru_family_lossdx((hipStream_t)stream, m, a);
}

// DPDs of the one-launch cascade step: the float GRU family, the float delta-GRU backbones and the plain LSTM (gru_cascade.hip)
static bool cascade_dpd_family(const odpd_model_t* m) {
    // (family_of answers FAM_GRU2 for ODPD_FLAG_TWO_LAYERS descriptors — the one-launch step only knows one-layer parameter layouts, so a
    // two-layer lstm must not slip in through its backbone id: ADVICE r04)
    return family_of(m) == FAM_GRU || (family_of(m) == FAM_DELTA && m->backbone != ODPD_DELTAJANET) ||
           (family_of(m) == FAM_LSTM && m->backbone == ODPD_LSTM) ||
           family_of(m) == FAM_QAT;      // (every quantised kind: gru, dgru, qgru, qgru_amp1, deltagru_tcnskip)
}
extern "C" int64_t odpd_cascade_rows(const odpd_model_t* dpd, const odpd_model_t* pa, int B, int T) {
    if (!model_ok(dpd) || !model_ok(pa) || B <= 0 || T <= 0) return ODPD_EINVAL;
    if (!cascade_dpd_family(dpd) || family_of(pa) != FAM_GRU || init_state(dpd) || init_state(pa)) return ODPD_EUNSUPPORTED;
    // a quantised DPD whose module is in eval() (ODPD_FLAG_EVAL: the 16-bit output quantiser of fc_out is active): the one-launch step
    // only carries the train-mode arithmetic, the chained launches honour the flag — so the step goes to them
    if (family_of(dpd) == FAM_QAT && (dpd->flags & ODPD_FLAG_EVAL)) return ODPD_EUNSUPPORTED;
    return gru_cascade_rows(dpd, pa, B, T);
}
extern "C" int odpd_cascade_fwd_bwd(void* stream, const odpd_model_t* dpd, const odpd_model_t* pa, int loss_kind, int B, int T, int64_t count,
                                    const float* dpd_params, const float* pa_params, const float* x, const float* target,
                                    const int64_t* frame_idx, int frame_stride, float* partials, double* dpd_stats) {
    if (!model_ok(dpd) || !model_ok(pa) || !dpd_params || !pa_params || !x || !target || !partials || B <= 0 || T <= 0 || count <= 0)
        return ODPD_EINVAL;
    if (!cascade_dpd_family(dpd) || family_of(pa) != FAM_GRU || init_state(dpd) || init_state(pa)) return ODPD_EUNSUPPORTED;
    CascArgs a{};
    a.thx = dpd->thx; a.thh = dpd->thh; a.stats = dpd_stats; a.bits_w = dpd->bits_w; a.bits_a = dpd->bits_a;
    a.dpd_params = dpd_params; a.pa_params = pa_params; a.x = x; a.target = target; a.partials = partials;
    a.frame_idx = reinterpret_cast<const long long*>(frame_idx); a.frame_stride = frame_stride;
    a.inv_count = (float)(1.0 / (double)count); a.loss_kind = loss_kind; a.B = B; a.T = T; a.Hd = dpd->hidden; a.Hp = pa->hidden;
    return gru_cascade_train((hipStream_t)stream, dpd, pa, a);
}

namespace {
// backbones whose fused train kernel addresses frames inside resident streams (SeqArgs::frame_idx) at every batch shape
inline bool framed_train_ok(const odpd_model_t* m) {
    return route_of(m) == ROUTE_NONE && (family_of(m) == FAM_GRU || family_of(m) == FAM_GMP || family_of(m) == FAM_RVTDCNN);
}
// ... for this batch shape: also the one-sequence-per-wave fused kernels of the other families (the large-batch kernel of lstm / vdlstm takes tensors)
inline bool framed_train_ok_shape(const odpd_model_t* m, int B, int T) {
    const FusedStep f = fused_step(m, B, T);
    return f.train && f.framed;
}
// bf16 sample storage is read by the float GRU family's fused train kernels (stage_in / ld_iq); every other path wants fp32 streams
inline bool frames_format_ok(const odpd_model_t* m, const odpd_frames_t* fr) {
    if (fr->sample_format == ODPD_SAMPLES_F32) return true;
    return fr->sample_format == ODPD_SAMPLES_BF16 && family_of(m) == FAM_GRU;
}
}  // namespace
extern "C" int odpd_framed_train_supported(const odpd_model_t* m) { return model_ok(m) && framed_train_ok(m) ? 1 : 0; }
extern "C" int odpd_framed_train_supported_shape(const odpd_model_t* m, int B, int T) {
    return model_ok(m) && B > 0 && T > 0 && framed_train_ok_shape(m, B, T) ? 1 : 0;
}

// odpd_train_fwd_bwd on frames addressed inside resident streams (no materialised (B,T,2) tensors): batch = the B frames
// fr->order[first .. first+B).  The caller finishes the step as usual (reduce, all-reduce when sharded, clip + AdamW).
extern "C" int odpd_train_fwd_bwd_framed(void* stream, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr,
                                         int64_t first, int B, int64_t count, const float* params, float* partials,
                                         float* workspace) {
    if (!model_ok(m) || !fr || !fr->x_stream || !fr->y_stream || !fr->order || fr->frame_length <= 0 || fr->stride <= 0 ||
        first < 0 || B <= 0 || first + B > fr->n_frames || count <= 0 || !params || !partials)
        return ODPD_EINVAL;
    const int T = fr->frame_length;
    const FusedStep f = fused_step(m, B, T);
    if (!f.train || !f.framed || !frames_format_ok(m, fr)) return ODPD_EUNSUPPORTED;
    // (only here, and only for the float GRU family's checkpoints: a NULL workspace is refused in front of the launcher — odpd_train_fwd_bwd
    // leaves it to the launcher, and the quantised step takes NULL where one checkpoint does: qat_s16.hip)
    if (f.ws == WS_CKPT && !workspace && family_of(m) == FAM_GRU) return ODPD_EINVAL;
    SeqArgs a = make_args(m, B, T);
    a.params = params; a.x = fr->x_stream; a.target = fr->y_stream; a.partials = partials;
    a.frame_idx = (const long long*)(fr->order + first); a.frame_stride = fr->stride; a.frames_bf16 = fr->sample_format == ODPD_SAMPLES_BF16;
    a.inv_count = (float)(1.0 / (double)count); a.loss_kind = loss_kind;
    set_workspace(a, f, workspace);
    return f.train((hipStream_t)stream, m, a);
}

// rank `rank` of `world` takes items [lo, hi) of n: contiguous shares, the first n % world ranks one item more
extern "C" void odpd_shard_range(int64_t n, int rank, int world, int64_t* lo, int64_t* hi) {
    const int64_t base = n / world, rem = n % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
}
// the tail of every data-parallel step: all-reduce of grad[0 .. P+4) over `comm` (NULL = one process), then clip + optimiser
// (opt_kind < 0: AdamW with the given hyper-parameters, else an enum odpd_optimizer kind).  A one-shot communicator's exchange runs as
// the optimiser kernel's prologue (one launch for both); RCCL's all-reduce is enqueued in front of it.
static int dp_clip_step(hipStream_t st, void* comm, int opt_kind, int64_t P, float* params, float* grad, float* state1, float* state2,
                        int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, float* norm_out,
                        float* loss_out, float inv_count, const unsigned char* skip) {
    XchgDev xd;
    const XchgDev* xp = nullptr;
    if (comm) {
        if (tuning().xchg_fused && comm_next_xchg(comm, P + kLossCols, &xd)) xp = &xd;
        else if (int rc = comm_allreduce(st, comm, grad, P + kLossCols)) return rc;
    }
    const int rc = opt_kind < 0 ? launch_clip_adamw(st, P, params, grad, state1, state2, step, lr, beta1, beta2, eps, weight_decay, max_norm, norm_out,
                                                    loss_out, inv_count, skip, xp)
                                : launch_clip_optim(st, opt_kind, P, params, grad, state1, state2, step, lr, max_norm, norm_out, loss_out, inv_count, skip, xp);
    if (rc != 0 && xp) comm_xchg_rollback(comm);      // the launch that was to carry the exchange failed: stay in step with the peers
    return rc;
}
extern "C" int odpd_clip_optim_step_dp(void* stream, void* comm, int opt_kind, int64_t P, float* params, float* grad, float* state1, float* state2,
                                       int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                       float* norm_out, const unsigned char* skip) {
    if (opt_kind > ODPD_OPT_RMSPROP) return ODPD_EINVAL;
    return dp_clip_step((hipStream_t)stream, comm, opt_kind < 0 ? -1 : opt_kind, P, params, grad, state1, state2, step, lr, beta1, beta2, eps,
                        weight_decay, max_norm, norm_out, nullptr, 0.0f, skip);
}

// ---- the native epoch loops: every step of an epoch issued back to back from C++, no host synchronisation, no Python between steps.  One driver:
// epoch_frames_ok, epoch_shapes_served (an epoch that will be refused launches nothing), epoch_steps (batch and shard arithmetic), run_epoch ----
namespace {
// frames order[f0 .. f0 + B) of the two streams gathered into (B,T,2) tensors (what IQFrameDataset + the DataLoader's collate build)
__global__ void gather_frames_kernel(const float2* __restrict__ xs, const float2* __restrict__ ys, const long long* __restrict__ order,
                                     int stride, int B, int T, float2* __restrict__ xo, float2* __restrict__ yo) {
    const long long n = (long long)B * T;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / T), t = (int)(i % T);
        const long long src = order[b] * stride + t;
        xo[i] = xs[src]; yo[i] = ys[src];
    }
}
// grad[P] = mean loss * count: the loss travels with the gradient (column P) exactly as in the Python-driven step
__global__ void loss_sum_kernel(float* grad_p, const float* loss_mean, float count) { grad_p[0] = loss_mean[0] * count; }
// an odpd_frames_t as an epoch loop takes it.  need_order: the loop visits the frames in fr->order (the sweeps take one order per run)
inline bool epoch_frames_ok(const odpd_frames_t* fr, int batch, bool need_order) {
    return fr && fr->x_stream && fr->y_stream && (fr->order || !need_order) && fr->n_frames > 0 && fr->frame_length > 0 && fr->stride > 0 && batch > 0;
}
struct EpochStep {
    int64_t i, f0;         // index of the step; position in `order` of the first frame of its global batch
    int64_t GB, lo, hi;    // size of the global batch (the last one may be short); this rank's frames [lo, hi) of it
    int B;                 // = hi - lo; 0: an empty shard of a short last batch
    int64_t count;         // GB * T * 2: the loss is a mean over the GLOBAL batch ...
    float inv_count;       // ... and its gradient is scaled by 1 / count
};
// body(step) for every step of an epoch in global batches of `batch`, each sharded over `world` ranks (one process: 0 of 1); a non-zero return ends it
template <class Body>
inline int epoch_steps(const odpd_frames_t* fr, int batch, int rank, int world, Body&& body) {
    const int64_t n = fr->n_frames;
    EpochStep s;
    for (s.f0 = 0, s.i = 0; s.f0 < n; s.f0 += batch, ++s.i) {
        s.GB = (n - s.f0) < batch ? (n - s.f0) : batch;
        odpd_shard_range(s.GB, rank, world, &s.lo, &s.hi);
        s.B = (int)(s.hi - s.lo);
        s.count = s.GB * fr->frame_length * 2;
        s.inv_count = (float)(1.0 / (double)s.count);
        if (int rc = body(s)) return rc;
    }
    return 0;
}
// every (shard of a) batch of the epoch — the full ones and the tail — must be served: served(B) for this rank's share of both
template <class Served>
inline bool epoch_shapes_served(const odpd_frames_t* fr, int batch, int rank, int world, Served&& served) {
    const int64_t full = fr->n_frames < batch ? fr->n_frames : batch, tail = fr->n_frames % batch;
    for (int64_t gb : {full, tail}) {
        if (!gb) continue;
        int64_t lo, hi;
        odpd_shard_range(gb, rank, world, &lo, &hi);
        if (hi > lo && !served((int)(hi - lo))) return false;
    }
    return true;
}
// how a step ends: the rows its launches left in `partials` summed into grad[0 .. P+4), then dp_clip_step (whose arguments these are)
struct StepTail {
    void* comm;                   // NULL: one process
    int opt_kind; int64_t P;
    float *params, *grad, *state1, *state2;
    double lr, beta1, beta2, eps, weight_decay, max_norm;
    const unsigned char* skip;    // NULL: every parameter is stepped
    float* partials;
    const float* loss_mean;       // the split chain: its loss kernel leaves the batch's mean loss here, not in column P of the rows (else NULL)
};
// One epoch.  Refused up front (ODPD_EUNSUPPORTED) unless served(B) holds for every batch shape of it; then per step launch(step, &rows) —
// forward + loss + backward of this rank's frames, `rows` partial-gradient rows — and the step's tail; losses_out[i] = mean loss of batch i.
template <class Served, class Launch>
inline int run_epoch(hipStream_t st, const odpd_frames_t* fr, int batch, int64_t first_step, const StepTail& t, float* losses_out,
                     Served&& served, Launch&& launch) {
    const int rank = t.comm ? comm_rank(t.comm) : 0, world = t.comm ? comm_world(t.comm) : 1;
    if (!epoch_shapes_served(fr, batch, rank, world, served)) return ODPD_EUNSUPPORTED;
    return epoch_steps(fr, batch, rank, world, [&](const EpochStep& s) -> int {
        if (s.B > 0) {
            int64_t rows = 0;
            if (int rc = launch(s, &rows)) return rc;
            if (int rc = odpd_reduce_partials(st, rows, t.P, t.partials, t.grad, 0)) return rc;
            if (t.loss_mean) hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1), 0, st, t.grad + t.P, t.loss_mean, (float)s.count);
        } else if (int rc = (int)hipMemsetAsync(t.grad, 0, (size_t)(t.P + kLossCols) * sizeof(float), st)) {
            return rc;      // (an empty shard of a short last batch: zeros into the sum)
        }
        return dp_clip_step(st, t.comm, t.opt_kind, t.P, t.params, t.grad, t.state1, t.state2, first_step + s.i, t.lr, t.beta1, t.beta2, t.eps,
                            t.weight_decay, t.max_norm, nullptr, losses_out + s.i, s.inv_count, t.skip);
    });
}
}  // namespace
// Native epoch loop (replaces the Python `for batch in loader` of net_train, train_funcs.py:28-48, for a single
// backbone with a fused kernel): every step = fused fwd+loss+bwd on frames addressed inside the resident streams,
// reduction, clip + AdamW; three launches per step.  losses_out[i] = mean loss of batch i (device).
// opt_kind < 0: AdamW with the given hyper-parameters; otherwise an enum odpd_optimizer kind with project.py's own.
// comm != NULL: every global batch sharded over the communicator's ranks, one all-reduce of grad[0 .. P+4) per step
static int train_epoch_impl(void* stream, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr, int batch, float* params, float* grad,
                            float* state1, float* state2, int64_t first_step, int opt_kind, double lr, double beta1, double beta2, double eps,
                            double weight_decay, double max_norm, float* partials, float* workspace, float* losses_out, void* comm = nullptr) {
    if (!model_ok(m) || !epoch_frames_ok(fr, batch, true) || !params || !grad || !state1 || !state2 || !partials || !losses_out || first_step <= 0)
        return ODPD_EINVAL;
    if (!frames_format_ok(m, fr)) return ODPD_EUNSUPPORTED;      // (bf16 frames: the float GRU family)
    const int T = fr->frame_length;
    const StepTail tail{comm, opt_kind, odpd_param_count(m), params, grad, state1, state2, lr, beta1, beta2, eps, weight_decay, max_norm,
                        /*skip*/ nullptr, partials, nullptr};
    return run_epoch((hipStream_t)stream, fr, batch, first_step, tail, losses_out, [&](int B) { return framed_train_ok_shape(m, B, T); },
                     [&](const EpochStep& s, int64_t* rows) -> int {
                         *rows = odpd_partial_rows(m, s.B, T, 1);
                         if (*rows <= 0) return *rows < 0 ? (int)*rows : ODPD_EUNSUPPORTED;
                         return odpd_train_fwd_bwd_framed(stream, m, loss_kind, fr, s.f0 + s.lo, s.B, s.count, params, partials, workspace);
                     });
}
extern "C" int odpd_train_epoch(void* stream, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr, int batch,
                                float* params, float* grad, float* exp_avg, float* exp_avg_sq, int64_t first_step, double lr,
                                double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                float* partials, float* workspace, float* losses_out) {
    return train_epoch_impl(stream, m, loss_kind, fr, batch, params, grad, exp_avg, exp_avg_sq, first_step, -1, lr, beta1, beta2, eps, weight_decay,
                            max_norm, partials, workspace, losses_out);
}
extern "C" int odpd_train_epoch_dp(void* stream, void* comm, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr, int batch, int opt_kind,
                                   float* params, float* grad, float* state1, float* state2, int64_t first_step, double lr, double beta1,
                                   double beta2, double eps, double weight_decay, double max_norm, float* partials, float* workspace,
                                   float* losses_out) {
    if (!comm || opt_kind > ODPD_OPT_RMSPROP) return ODPD_EINVAL;
    return train_epoch_impl(stream, m, loss_kind, fr, batch, params, grad, state1, state2, first_step, opt_kind < 0 ? -1 : opt_kind, lr, beta1, beta2,
                            eps, weight_decay, max_norm, partials, workspace, losses_out, comm);
}
extern "C" int odpd_train_epoch_opt(void* stream, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr, int batch, int opt_kind,
                                    float* params, float* grad, float* state1, float* state2, int64_t first_step, double lr,
                                    double max_norm, float* partials, float* workspace, float* losses_out) {
    if (opt_kind < ODPD_OPT_ADAMW || opt_kind > ODPD_OPT_RMSPROP) return ODPD_EINVAL;
    return train_epoch_impl(stream, m, loss_kind, fr, batch, params, grad, state1, state2, first_step, opt_kind, lr, 0, 0, 0, 0, max_norm, partials,
                            workspace, losses_out);
}
// ---- native epoch loop of train_dpd at the reference's batch sizes: the one-launch cascade step (gru_cascade.hip) on frames read in place;
// comm != NULL: sharded as train_epoch_impl ----
extern "C" int odpd_train_epoch_cascade(void* stream, void* comm, const odpd_model_t* dpd, const odpd_model_t* pa, int loss_kind,
                                        const odpd_frames_t* fr, int batch, int opt_kind, float* dpd_params, const float* pa_params, float* grad,
                                        float* state1, float* state2, int64_t first_step, double lr, double beta1, double beta2, double eps,
                                        double weight_decay, double max_norm, const unsigned char* skip, float* partials, double* dpd_stats,
                                        float* losses_out) {
    if (!model_ok(dpd) || !model_ok(pa) || !epoch_frames_ok(fr, batch, true) || !dpd_params || !pa_params || !grad || !state1 || !state2 ||
        !partials || !losses_out || first_step <= 0 || opt_kind > ODPD_OPT_RMSPROP)
        return ODPD_EINVAL;
    if (fr->sample_format != ODPD_SAMPLES_F32) return ODPD_EUNSUPPORTED;
    const int T = fr->frame_length;
    const StepTail tail{comm, opt_kind, odpd_param_count(dpd), dpd_params, grad, state1, state2, lr, beta1, beta2, eps, weight_decay, max_norm,
                        skip, partials, nullptr};
    return run_epoch((hipStream_t)stream, fr, batch, first_step, tail, losses_out, [&](int B) { return odpd_cascade_rows(dpd, pa, B, T) > 0; },
                     [&](const EpochStep& s, int64_t* rows) -> int {
                         *rows = odpd_cascade_rows(dpd, pa, s.B, T);
                         return odpd_cascade_fwd_bwd(stream, dpd, pa, loss_kind, s.B, T, s.count, dpd_params, pa_params, fr->x_stream, fr->y_stream,
                                                     fr->order + s.f0 + s.lo, fr->stride, partials, dpd_stats);
                     });
}
// ---- native epoch loop for backbones without a fused train kernel at this shape (the split chain of train_funcs.py:33-44: gather, forward,
// loss, backward per step); one process, and not the state route ----
extern "C" int odpd_train_epoch_split(void* stream, const odpd_model_t* m, int loss_kind, const odpd_frames_t* fr, int batch, int opt_kind,
                                      float* params, float* grad, float* state1, float* state2, int64_t first_step, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, double max_norm, const unsigned char* skip,
                                      float* xbuf, float* tbuf, float* ybuf, float* dybuf, float* ckpt, float* partials, float* loss_scratch,
                                      double* stats, float* losses_out) {
    if (!model_ok(m) || !epoch_frames_ok(fr, batch, true) || !params || !grad || !state1 || !state2 || !xbuf || !tbuf || !ybuf || !dybuf ||
        !partials || !loss_scratch || !losses_out || first_step <= 0 || opt_kind > ODPD_OPT_RMSPROP)
        return ODPD_EINVAL;
    if (fr->sample_format != ODPD_SAMPLES_F32 || init_state(m)) return ODPD_EUNSUPPORTED;
    const int T = fr->frame_length;
    const int64_t P = odpd_param_count(m);
    if (P <= 0) return P < 0 ? (int)P : ODPD_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const StepTail tail{/*comm*/ nullptr, opt_kind, P, params, grad, state1, state2, lr, beta1, beta2, eps, weight_decay, max_norm,
                        skip, partials, /*loss_mean*/ loss_scratch};
    return run_epoch(st, fr, batch, first_step, tail, losses_out, [&](int B) { return odpd_partial_rows(m, B, T, 0) > 0; },
                     [&](const EpochStep& s, int64_t* rows) -> int {
                         *rows = odpd_partial_rows(m, s.B, T, 0);
                         if (*rows <= 0) return *rows < 0 ? (int)*rows : ODPD_EUNSUPPORTED;
                         const long long work = (long long)s.B * T;
                         const int grid = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
                         hipLaunchKernelGGL(gather_frames_kernel, dim3(grid), dim3(256), 0, st, (const float2*)fr->x_stream,
                                            (const float2*)fr->y_stream, (const long long*)(fr->order + s.f0), fr->stride, s.B, T, (float2*)xbuf,
                                            (float2*)tbuf);
                         if (int rc = (int)hipGetLastError()) return rc;
                         if (int rc = odpd_backbone_fwd(stream, m, s.B, T, params, xbuf, ybuf, ckpt, stats)) return rc;
                         if (int rc = odpd_loss_fwd_bwd(stream, loss_kind, s.count, s.count, ybuf, tbuf, dybuf, loss_scratch)) return rc;
                         return odpd_backbone_bwd(stream, m, s.B, T, params, xbuf, dybuf, ckpt, partials, nullptr);
                     });
}
// ---- lockstep sweeps: K independent runs of ONE model shape (the seeds of bash_scripts/train_all_pa.sh:26-57) advance together — per step
// one fused train launch of K x grid workgroups, one row reduction, one clip + AdamW launch; each run bit-identical to its solo epoch.
// scratch: run table | PA parameter pointers (the cascade sweeps only) | K threshold pairs (the cascade threshold sweep only) | K step sizes per
// step of the epoch ----
namespace {
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t sweep_pa_off(int K) { return align256((size_t)K * sizeof(SweepRun)); }
inline size_t sweep_th_off(int K) { return sweep_pa_off(K) + align256((size_t)K * sizeof(float*)); }      // (behind the PA table)
inline size_t sweep_ss_off(int K, bool pa_table, bool th_table = false) {
    return sweep_pa_off(K) + (pa_table ? align256((size_t)K * sizeof(float*)) : 0) + (th_table ? align256((size_t)K * 2 * sizeof(float)) : 0);
}
inline int64_t sweep_scratch_bytes(int K, int64_t n_steps, bool pa_table, bool th_table = false) {
    if (K <= 0 || n_steps < 0) return ODPD_EINVAL;
    return (int64_t)sweep_ss_off(K, pa_table, th_table) + (int64_t)K * n_steps * (int64_t)sizeof(float) + 256;
}
// the pointers every run of a training sweep needs, and extra(k) on top of them
template <class Extra>
inline bool sweep_runs_ok(int K, const odpd_sweep_run_t* runs, Extra&& extra) {
    for (int k = 0; k < K; ++k)
        if (const odpd_sweep_run_t& r = runs[k]; !r.params || !r.grad || !r.exp_avg || !r.exp_avg_sq || !r.partials || !r.losses_out || !r.order || !extra(k))
            return false;
    return true;
}
inline int upload_sweep(hipStream_t st, int K, const odpd_sweep_run_t* runs, double weight_decay, void* scratch, SweepRun** dev_out) {
    std::vector<SweepRun> h((size_t)K);
    for (int k = 0; k < K; ++k) {
        const odpd_sweep_run_t& r = runs[k];
        SweepRun& d = h[(size_t)k];
        d.params = r.params; d.grad = r.grad; d.state1 = r.exp_avg; d.state2 = r.exp_avg_sq; d.partials = r.partials; d.losses = r.losses_out;
        d.y = r.y; d.workspace = r.workspace; d.order = (const long long*)r.order; d.decay = (float)(1.0 - r.lr * weight_decay); d.pad = 0.0f;
    }
    *dev_out = reinterpret_cast<SweepRun*>(scratch);
    return (int)hipMemcpyAsync(scratch, h.data(), (size_t)K * sizeof(SweepRun), hipMemcpyHostToDevice, st);      // (pageable source: staged before the call returns)
}
// per-step, per-run step sizes lr_k / (1 - beta1^step) of an epoch, at ss_dev: double arithmetic rounded once, exactly launch_clip_adamw's
inline int sweep_step_sizes(hipStream_t st, int K, const odpd_sweep_run_t* runs, int64_t n_steps, int64_t first_step, double beta1, float* ss_dev) {
    std::vector<float> ss((size_t)(K * n_steps));
    for (int64_t i = 0; i < n_steps; ++i) {
        const double bc1 = 1.0 - pow(beta1, (double)(first_step + i));
        for (int k = 0; k < K; ++k) ss[(size_t)(i * K + k)] = (float)(runs[k].lr / bc1);
    }
    return (int)hipMemcpyAsync(ss_dev, ss.data(), ss.size() * sizeof(float), hipMemcpyHostToDevice, st);      // (pageable source, as above)
}
// One lockstep epoch: the run table, every run's PA parameter pointer (pa_params; NULL: no such table), every run's threshold pair (thresholds,
// K x 2 floats behind the PA table; NULL: no such table) and the step sizes into `scratch`, then per step
// launch(step, run table, PA table, threshold table or NULL, &rows) — the K runs' forward + loss + backward — one row reduction, one clip + AdamW launch
template <class Launch>
inline int run_sweep_epoch(hipStream_t st, int K, const odpd_sweep_run_t* runs, const float* const* pa_params, const float* thresholds,
                           const odpd_frames_t* fr, int batch, int64_t P, int64_t first_step, double beta1, double beta2, double eps,
                           double weight_decay, double max_norm, void* scratch, Launch&& launch) {
    SweepRun* dev = nullptr;
    if (int rc = upload_sweep(st, K, runs, weight_decay, scratch, &dev)) return rc;
    const float** pa_dev = reinterpret_cast<const float**>(reinterpret_cast<char*>(scratch) + sweep_pa_off(K));
    if (pa_params) ODPD_CHECK_HIP(hipMemcpyAsync(pa_dev, pa_params, (size_t)K * sizeof(float*), hipMemcpyHostToDevice, st));      // (pageable source, as above)
    float* th_dev = thresholds ? reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + sweep_th_off(K)) : nullptr;
    if (th_dev) ODPD_CHECK_HIP(hipMemcpyAsync(th_dev, thresholds, (size_t)K * 2 * sizeof(float), hipMemcpyHostToDevice, st));      // (pageable source, as above)
    float* ss_dev = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + sweep_ss_off(K, pa_params != nullptr, thresholds != nullptr));
    if (int rc = sweep_step_sizes(st, K, runs, (fr->n_frames + batch - 1) / batch, first_step, beta1, ss_dev)) return rc;
    return epoch_steps(fr, batch, 0, 1, [&](const EpochStep& s) -> int {
        int64_t rows = 0;
        if (int rc = launch(s, dev, pa_dev, th_dev, &rows)) return rc;
        if (int rc = launch_reduce_sweep(st, dev, K, rows, P)) return rc;
        return launch_clip_adamw_sweep(st, dev, K, P, ss_dev + s.i * K, first_step + s.i, s.i, beta1, beta2, eps, max_norm, s.inv_count);
    });
}
}  // namespace
extern "C" int64_t odpd_sweep_scratch_bytes(int K, int64_t n_steps) { return sweep_scratch_bytes(K, n_steps, false); }
extern "C" int odpd_sweep_train_supported(const odpd_model_t* m, int B, int T) {
    return model_ok(m) && gru_family_model(m) && gru_sweep_train_ok(m, B, T) ? 1 : 0;
}
extern "C" int odpd_sweep_fwd_supported(const odpd_model_t* m, int B, int T) {
    return model_ok(m) && gru_family_model(m) && gru_sweep_eval_ok(m, B, T) ? 1 : 0;
}
extern "C" int odpd_sweep_s16_supported(const odpd_model_t* m) {
    return model_ok(m) && gru_family_model(m) && gru_s16_sweep_ok(m) ? 1 : 0;
}
extern "C" int64_t odpd_sweep_partial_rows(const odpd_model_t* m, int B, int T, int flags) {
    if (!model_ok(m) || B <= 0 || T <= 0 || !gru_family_model(m)) return ODPD_EUNSUPPORTED;
    if (flags & ODPD_SWEEP_S16) return gru_s16_sweep_ok(m) ? gru_s16_rows(m, B) : (int64_t)ODPD_EUNSUPPORTED;
    return gru_sweep_train_ok(m, B, T) ? gru_sweep_train_rows(m, B, T) : (int64_t)ODPD_EUNSUPPORTED;
}
extern "C" int64_t odpd_sweep_workspace_floats(const odpd_model_t* m, int B, int T, int flags) {
    if (!model_ok(m) || B <= 0 || T <= 0) return ODPD_EINVAL;
    if (init_state(m) || quant_cell(m)) return ODPD_EUNSUPPORTED;
    if (!(flags & ODPD_SWEEP_S16)) return 0;
    return odpd_sweep_s16_supported(m) ? gru_s16_train_ws_floats(m, B, T) : (int64_t)ODPD_EUNSUPPORTED;
}
extern "C" int odpd_train_epoch_sweep(void* stream, const odpd_model_t* m, int K, const odpd_sweep_run_t* runs, int loss_kind, const odpd_frames_t* fr,
                                      int batch, int64_t first_step, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                      int flags, void* scratch) {
    if (!model_ok(m) || K <= 0 || !runs || !epoch_frames_ok(fr, batch, false) || first_step <= 0 || !scratch) return ODPD_EINVAL;
    if (!sweep_runs_ok(K, runs, [](int) { return true; })) return ODPD_EINVAL;
    const int T = fr->frame_length;
    const bool s16 = (flags & ODPD_SWEEP_S16) != 0;
    if (!gru_family_model(m) || !frames_format_ok(m, fr)) return ODPD_EUNSUPPORTED;      // (bf16 frames: served)
    if (s16) {      // the 16-sequences-per-wave kernel: any batch shape, checkpoints in every run's workspace
        if (!gru_s16_sweep_ok(m)) return ODPD_EUNSUPPORTED;
        for (int k = 0; k < K; ++k)
            if (!runs[k].workspace) return ODPD_EINVAL;
    } else if (!epoch_shapes_served(fr, batch, 0, 1, [&](int B) { return gru_sweep_train_ok(m, B, T); })) {
        return ODPD_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    return run_sweep_epoch(st, K, runs, /*pa_params*/ nullptr, /*thresholds*/ nullptr, fr, batch, odpd_param_count(m), first_step, beta1, beta2, eps,
                           weight_decay, max_norm, scratch, [&](const EpochStep& s, SweepRun* dev, const float**, const float*, int64_t* rows) -> int {
                               SeqArgs a = make_args(m, s.B, T);
                               a.x = fr->x_stream; a.target = fr->y_stream; a.frame_stride = fr->stride; a.inv_count = s.inv_count;
                               a.frames_bf16 = fr->sample_format == ODPD_SAMPLES_BF16; a.loss_kind = loss_kind;
                               if (s16) a.nck = num_ckpt(T);
                               *rows = s16 ? gru_s16_rows(m, s.B) : gru_sweep_train_rows(m, s.B, T);
                               return s16 ? gru_s16_sweep_train(st, m, a, dev, K, (long long)s.f0) : gru_sweep_train(st, m, a, dev, K, (long long)s.f0);
                           });
}
// ---- lockstep train_dpd sweeps (the seeds of bash_scripts/train_all_dpd.sh): K runs of one float (DPD, PA) pair on the one-launch cascade step.
// The step gives every frame a workgroup with a CU('s LDS) to itself, so at batch 64 one run leaves three quarters of the chip idle: here
// the launch that fills the chip IS the bit-exact one (workgroups of different runs never interact) ----
extern "C" int odpd_sweep_cascade_supported(const odpd_model_t* dpd, const odpd_model_t* pa, int B, int T) {
    if (!dpd || !pa || !model_ok(dpd) || !model_ok(pa) || dpd->bits_w != 0) return 0;
    if (family_of(dpd) == FAM_QAT) return 0;
    return odpd_cascade_rows(dpd, pa, B, T) > 0 ? 1 : 0;
}
extern "C" int64_t odpd_sweep_cascade_scratch_bytes(int K, int64_t n_steps) { return sweep_scratch_bytes(K, n_steps, true); }
// both cascade sweep entry points; thresholds (HOST, K x 2; NULL: the descriptor's pair for every run) and th_call tell them apart
static int cascade_sweep_epoch(void* stream, const odpd_model_t* dpd, const odpd_model_t* pa, int K, const odpd_sweep_run_t* runs,
                               const float* const* pa_params, const float* thresholds, bool th_call, int loss_kind, const odpd_frames_t* fr,
                               int batch, int64_t first_step, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                               void* scratch) {
    if (!dpd || !pa || !model_ok(dpd) || !model_ok(pa) || K <= 0 || !runs || !pa_params || !epoch_frames_ok(fr, batch, false) || first_step <= 0 ||
        !scratch || (th_call && !thresholds))
        return ODPD_EINVAL;
    // (on top of the common pointers: every run's PA; workspace = a delta DPD's sparsity counters — doubles — or NULL)
    if (!sweep_runs_ok(K, runs, [&](int k) { return pa_params[k] && !(reinterpret_cast<uintptr_t>(runs[k].workspace) & 7); })) return ODPD_EINVAL;
    if (th_call)      // (|delta| < threshold masks the delta: finite and not negative)
        for (int i = 0; i < 2 * K; ++i)
            if (!std::isfinite(thresholds[i]) || thresholds[i] < 0.0f) return ODPD_EINVAL;
    if (fr->sample_format != ODPD_SAMPLES_F32) return ODPD_EUNSUPPORTED;
    const int T = fr->frame_length;
    if (!epoch_shapes_served(fr, batch, 0, 1, [&](int B) {
            return (th_call ? odpd_sweep_cascade_th_supported(dpd, pa, B, T) : odpd_sweep_cascade_supported(dpd, pa, B, T)) != 0;
        }))
        return ODPD_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    CascArgs a{};
    a.thx = dpd->thx; a.thh = dpd->thh; a.bits_w = dpd->bits_w; a.bits_a = dpd->bits_a;      // (a threshold sweep: the kernel overwrites the pair per run)
    a.x = fr->x_stream; a.target = fr->y_stream; a.frame_stride = fr->stride;
    a.loss_kind = loss_kind; a.T = T; a.Hd = dpd->hidden; a.Hp = pa->hidden;
    return run_sweep_epoch(st, K, runs, pa_params, thresholds, fr, batch, odpd_param_count(dpd), first_step, beta1, beta2, eps, weight_decay, max_norm,
                           scratch, [&](const EpochStep& s, SweepRun* dev, const float** pa_dev, const float* th_dev, int64_t* rows) -> int {
                               a.B = s.B; a.inv_count = s.inv_count;
                               *rows = odpd_cascade_rows(dpd, pa, s.B, T);
                               return gru_cascade_sweep_train(st, dpd, pa, a, dev, pa_dev, th_dev, K, (long long)s.f0);
                           });
}
extern "C" int odpd_train_epoch_cascade_sweep(void* stream, const odpd_model_t* dpd, const odpd_model_t* pa, int K, const odpd_sweep_run_t* runs,
                                              const float* const* pa_params, int loss_kind, const odpd_frames_t* fr, int batch, int64_t first_step,
                                              double beta1, double beta2, double eps, double weight_decay, double max_norm, void* scratch) {
    return cascade_sweep_epoch(stream, dpd, pa, K, runs, pa_params, /*thresholds*/ nullptr, false, loss_kind, fr, batch, first_step, beta1, beta2, eps,
                               weight_decay, max_norm, scratch);
}
// ---- ... with a pair of delta thresholds per run (the THX / THH knobs of bash_scripts/OpenDPDv2.sh): deltagru / deltagru_tcnskip DPDs only;
// the pairs travel behind the PA pointer table and are read once per workgroup ----
extern "C" int odpd_sweep_cascade_th_supported(const odpd_model_t* dpd, const odpd_model_t* pa, int B, int T) {
    if (!odpd_sweep_cascade_supported(dpd, pa, B, T)) return 0;
    return dpd->backbone == ODPD_DELTAGRU || dpd->backbone == ODPD_TRES_DELTAGRU ? 1 : 0;
}
extern "C" int64_t odpd_sweep_cascade_th_scratch_bytes(int K, int64_t n_steps) { return sweep_scratch_bytes(K, n_steps, true, true); }
extern "C" int odpd_train_epoch_cascade_sweep_th(void* stream, const odpd_model_t* dpd, const odpd_model_t* pa, int K, const odpd_sweep_run_t* runs,
                                                 const float* const* pa_params, const float* thresholds, int loss_kind, const odpd_frames_t* fr,
                                                 int batch, int64_t first_step, double beta1, double beta2, double eps, double weight_decay,
                                                 double max_norm, void* scratch) {
    return cascade_sweep_epoch(stream, dpd, pa, K, runs, pa_params, thresholds, true, loss_kind, fr, batch, first_step, beta1, beta2, eps, weight_decay,
                               max_norm, scratch);
}
extern "C" int odpd_backbone_fwd_sweep(void* stream, const odpd_model_t* m, int K, const odpd_sweep_run_t* runs, int B, int T, const float* x,
                                       void* scratch) {
    if (!model_ok(m) || K <= 0 || !runs || !x || B <= 0 || T <= 0 || !scratch) return ODPD_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!runs[k].params || !runs[k].y) return ODPD_EINVAL;
    if (!gru_family_model(m) || !gru_sweep_eval_ok(m, B, T)) return ODPD_EUNSUPPORTED;
    SweepRun* dev = nullptr;
    if (int rc = upload_sweep((hipStream_t)stream, K, runs, 0.0, scratch, &dev)) return rc;
    SeqArgs a = make_args(m, B, T);
    a.x = x;
    return gru_sweep_eval((hipStream_t)stream, m, a, dev, K);
}
