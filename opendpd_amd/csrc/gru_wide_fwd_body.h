// gru_wide_fwd_body.h — the body of wide_gru_fwd_kernel and wide_gru_fwd_state_kernel (gru_wide.hip), #included inside each with the
// kernel's template parameters FM, DG, SAVE and a constexpr S0 in scope (S0: the sequence starts from a.h0).  Not a header of its own.
    constexpr int F = FeatDim<FM>::F, NS = DG ? 6 : 5;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const GruLayout L = gru_layout(a.H, F, DG);
    const int H = L.H, T = a.T, OW = DG ? H + 6 : H;
    float* pl = smem;
    stage_params(pl, a.params, L.P);
    float* ftab = smem + pad4(L.P);            // [64][8]: features of the chunk's steps
    float* hb = ftab + kWC * 8;                // [64]: the state, for the broadcast reads
    float* hist = hb + 64;                     // [64][65]: h of the chunk's steps
    float* hist2 = hist + kWC * kWS;           // DG: [64][65] fc_hid pre-activations
    float* whp = hist2 + kWC * kWS;            // DG: fc_hid rows, zero padded to 64 columns
    const bool vo = lane < H;
    if constexpr (DG) {
        for (int i = lane; i < H * 64; i += 64) whp[i] = (i & 63) < H ? pl[L.o_w_hid + (i >> 6) * H + (i & 63)] : 0.0f;
    }
    float whh[3][64], wih[3][F], bi[3], bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
        for (int k = 0; k < 64; ++k) whh[g][k] = (vo && k < H) ? pl[L.o_w_hh + (g * H + lane) * H + k] : 0.0f;
#pragma unroll
        for (int i = 0; i < F; ++i) wih[g][i] = vo ? pl[L.o_w_ih + (g * H + lane) * F + i] : 0.0f;
        bi[g] = vo ? pl[L.o_b_ih + g * H + lane] : 0.0f;
        bh[g] = vo ? pl[L.o_b_hh + g * H + lane] : 0.0f;
    }
    wave_lds_fence();
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float2* xg = reinterpret_cast<const float2*>(a.x) + (size_t)b * T;
        float2* yg = reinterpret_cast<float2*>(a.y) + (size_t)b * T;
        float* sv = SAVE ? a.ckpt + (size_t)b * T * NS * 64 : nullptr;
        float h = 0.0f;
        if constexpr (S0) h = vo ? a.h0[(size_t)b * H + lane] : 0.0f;
        for (int t0 = 0; t0 < T; t0 += kWC) {
            const int len = min(kWC, T - t0);
            wave_lds_fence();
            wide_stage_features<FM>(ftab, xg, t0, T, lane);
            wave_lds_fence();
            for (int tt = 0; tt < len; ++tt) {
                hb[lane] = h;
                wave_lds_fence();
                float gh[3] = {bh[0], bh[1], bh[2]}, gi[3] = {bi[0], bi[1], bi[2]};
                const float4* hb4 = reinterpret_cast<const float4*>(hb);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float4 hv = hb4[q];
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        gh[g] = __builtin_fmaf(whh[g][4 * q], hv.x, gh[g]); gh[g] = __builtin_fmaf(whh[g][4 * q + 1], hv.y, gh[g]);
                        gh[g] = __builtin_fmaf(whh[g][4 * q + 2], hv.z, gh[g]); gh[g] = __builtin_fmaf(whh[g][4 * q + 3], hv.w, gh[g]);
                    }
                }
                const float4 f0 = reinterpret_cast<const float4*>(ftab)[2 * tt], f1 = reinterpret_cast<const float4*>(ftab)[2 * tt + 1];
                const float fe[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int i = 0; i < F; ++i) gi[g] = __builtin_fmaf(wih[g][i], fe[i], gi[g]);
                const float r = sigmoidf_(gi[0] + gh[0]), z = sigmoidf_(gi[1] + gh[1]);
                const float n = tanhf_(__builtin_fmaf(r, gh[2], gi[2]));
                const float hn = vo ? __builtin_fmaf(z, h - n, n) : 0.0f;            // (1 - z) n + z h
                if constexpr (SAVE) {
                    float* s = sv + (size_t)(t0 + tt) * NS * 64 + lane;
                    s[0] = r; s[64] = z; s[128] = n; s[192] = gh[2]; s[256] = hn;
                }
                h = hn;
                hist[tt * kWS + lane] = h;
                wave_lds_fence();
            }
            // the chunk's outputs, lane = time step
            if (lane < len) {
                const float* hr = hist + lane * kWS;
                float y0 = pl[L.o_b_out], y1 = pl[L.o_b_out + 1];
                if constexpr (!DG) {
                    for (int j = 0; j < H; ++j) {
                        const float hv = hr[j];
                        y0 = __builtin_fmaf(pl[L.o_w_out + j], hv, y0); y1 = __builtin_fmaf(pl[L.o_w_out + OW + j], hv, y1);
                    }
                } else {
                    float hrow[64];
#pragma unroll
                    for (int k = 0; k < 64; ++k) hrow[k] = hr[k];
                    for (int j = 0; j < H; ++j) {             // out = relu(fc_hid(h)) (dgru.py:71)
                        float acc = pl[L.o_b_hid + j];
                        const float4* w4 = reinterpret_cast<const float4*>(whp + j * 64);
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const float4 w = w4[q];
                            acc = __builtin_fmaf(w.x, hrow[4 * q], acc); acc = __builtin_fmaf(w.y, hrow[4 * q + 1], acc);
                            acc = __builtin_fmaf(w.z, hrow[4 * q + 2], acc); acc = __builtin_fmaf(w.w, hrow[4 * q + 3], acc);
                        }
                        hist2[lane * kWS + j] = acc;
                        const float o = __builtin_fmaxf(acc, 0.0f);
                        y0 = __builtin_fmaf(pl[L.o_w_out + j], o, y0); y1 = __builtin_fmaf(pl[L.o_w_out + OW + j], o, y1);
                    }
#pragma unroll
                    for (int i = 0; i < 6; ++i) {             // y = fc_out(cat(out, features)) (dgru.py:72-73)
                        const float fv = ftab[lane * 8 + i];
                        y0 = __builtin_fmaf(pl[L.o_w_out + H + i], fv, y0); y1 = __builtin_fmaf(pl[L.o_w_out + OW + H + i], fv, y1);
                    }
                }
                yg[t0 + lane] = make_float2(y0, y1);
            }
            if constexpr (DG && SAVE) {
                wave_lds_fence();
                for (int tt = 0; tt < len; ++tt) sv[(size_t)(t0 + tt) * NS * 64 + 320 + lane] = hist2[tt * kWS + lane];
            }
        }
        wave_lds_fence();
    }
