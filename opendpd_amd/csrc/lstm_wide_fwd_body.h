// lstm_wide_fwd_body.h — the body of wide_lstm_fwd_kernel and wide_lstm_fwd_state_kernel (lstm_wide.hip), #included inside each with
// the kernel's template parameter SAVE and a constexpr S0 in scope (S0: h and c start from a.h0).  Not a header of its own.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const LstmLayout L = lstm_layout(a.H, 0, a.bits_w > 0);
    const int H = L.H, T = a.T;
    float* pl = smem;
    stage_params(pl, a.params, L.P);
    float* xb = smem + pad4(L.P);              // [64][2]: I, Q of the chunk's steps
    float* hb = xb + kLC * 2;                  // [64]: the state, for the broadcast reads
    float* hist = hb + 64;                     // [64][65]: h of the chunk's steps
    float* wop = hist + kLC * kLS;             // [64][65]: gate o's W_hh rows, zero padded
    const bool vo = lane < H;
    for (int i = lane; i < 64 * kLS; i += 64) {
        const int j = i / kLS, k = i % kLS;
        wop[i] = (j < H && k < H) ? pl[L.o_w_hh + (3 * H + j) * H + k] : 0.0f;
    }
    // `--quant` (bits_w > 0; run-time, wave-uniform): fc_out is an INT_Linear (quant_layers.py:48-85) — its weights become their quantised
    // values in the staged copy, the chunk's states are quantised where the head reads them, ODPD_FLAG_EVAL adds the 16-bit output grid
    const bool qh = a.bits_w > 0;
    q16::Quant qa{1.0f, 1.0f, 0.0f, 0.0f}, qo{1.0f, 1.0f, 0.0f, 0.0f};
    if (qh) {
        const q16::Quant qw = q16::make_quant(pl[L.o_q_out], a.bits_w);
        qa = q16::make_quant(pl[L.o_q_out + 1], a.bits_a);
        qo = q16::make_quant(pl[L.o_q_out + 2], 16);
        wave_lds_fence();
        for (int i = lane; i < 2 * H; i += 64) pl[L.o_w_out + i] = q16::qapply(pl[L.o_w_out + i], qw);
        wave_lds_fence();
    }
    float whh[3][64], wih[4][2], bg[4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int k = 0; k < 64; ++k) whh[g][k] = (vo && k < H) ? pl[L.o_w_hh + (g * H + lane) * H + k] : 0.0f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wih[g][0] = vo ? pl[L.o_w_ih + (g * H + lane) * 2] : 0.0f;
        wih[g][1] = vo ? pl[L.o_w_ih + (g * H + lane) * 2 + 1] : 0.0f;
        bg[g] = vo ? pl[L.o_b_ih + g * H + lane] + pl[L.o_b_hh + g * H + lane] : 0.0f;
    }
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        float2* yg = reinterpret_cast<float2*>(a.y) + (size_t)b * T;
        float* sv = SAVE ? a.ckpt + (size_t)b * T * kLNS * 64 : nullptr;
        float h = 0.0f, c = 0.0f;
        if constexpr (S0) h = c = vo ? a.h0[(size_t)b * H + lane] : 0.0f;
        for (int t0 = 0; t0 < T; t0 += kLC) {
            const int len = min(kLC, T - t0);
            wave_lds_fence();
            reinterpret_cast<float2*>(xb)[lane] = t0 + lane < T ? xg[t0 + lane] : make_float2(0.0f, 0.0f);
            wave_lds_fence();
            for (int tt = 0; tt < len; ++tt) {
                hb[lane] = h;
                wave_lds_fence();
                const float2 xv = reinterpret_cast<const float2*>(xb)[tt];
                float pre[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = __builtin_fmaf(wih[g][1], xv.y, __builtin_fmaf(wih[g][0], xv.x, bg[g]));
                const float4* hb4 = reinterpret_cast<const float4*>(hb);
                const float* wo = wop + lane * kLS;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float4 hv = hb4[q];
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        pre[g] = __builtin_fmaf(whh[g][4 * q], hv.x, pre[g]); pre[g] = __builtin_fmaf(whh[g][4 * q + 1], hv.y, pre[g]);
                        pre[g] = __builtin_fmaf(whh[g][4 * q + 2], hv.z, pre[g]); pre[g] = __builtin_fmaf(whh[g][4 * q + 3], hv.w, pre[g]);
                    }
                    pre[3] = __builtin_fmaf(wo[4 * q], hv.x, pre[3]); pre[3] = __builtin_fmaf(wo[4 * q + 1], hv.y, pre[3]);
                    pre[3] = __builtin_fmaf(wo[4 * q + 2], hv.z, pre[3]); pre[3] = __builtin_fmaf(wo[4 * q + 3], hv.w, pre[3]);
                }
                const float gi = sigmoidf_(pre[0]), gf = sigmoidf_(pre[1]), gg = tanhf_(pre[2]), go = sigmoidf_(pre[3]);
                const float cn = vo ? __builtin_fmaf(gf, c, gi * gg) : 0.0f;
                const float hn = vo ? go * tanhf_(cn) : 0.0f;
                if constexpr (SAVE) {
                    float* s = sv + (size_t)(t0 + tt) * kLNS * 64 + lane;
                    s[0] = gi; s[64] = gf; s[128] = gg; s[192] = go; s[256] = cn; s[320] = hn;
                }
                c = cn; h = hn;
                hist[tt * kLS + lane] = h;
                wave_lds_fence();
            }
            if (lane < len) {      // the chunk's outputs, lane = time step
                const float* hr = hist + lane * kLS;
                float y0 = qh ? 0.0f : pl[L.o_b_out], y1 = qh ? 0.0f : pl[L.o_b_out + 1];
                for (int j = 0; j < H; ++j) {
                    const float hv = qh ? q16::qapply(hr[j], qa) : hr[j];
                    y0 = __builtin_fmaf(pl[L.o_w_out + j], hv, y0); y1 = __builtin_fmaf(pl[L.o_w_out + H + j], hv, y1);
                }
                if (qh) {      // grid sums first, then the float bias (F.linear(q_a(h), q_w(W), b))
                    y0 += pl[L.o_b_out]; y1 += pl[L.o_b_out + 1];
                    if (a.eval_out) { y0 = q16::qapply(y0, qo); y1 = q16::qapply(y1, qo); }
                }
                yg[t0 + lane] = make_float2(y0, y1);
            }
        }
        wave_lds_fence();
    }
