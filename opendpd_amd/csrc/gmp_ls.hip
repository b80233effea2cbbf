// gmp_ls.hip — the normal equations of the gmp backbone's least-squares fit (odpd_gmp_gram): G = A^T A in fp64 on v_mfma_f64_16x16x4_f64.
//
// gmp (gmp.hip, reference backbones/gmp.py:5-50) is linear in its 495 real weights.  For sequences x, target (B, T, 2) the real design
// matrix A has two rows per output sample (real part, imaginary part) and 496 columns: column j < 495 is the complex basis term that
// multiplies Weight[0, j] (gmp.py:41-46), column 495 the target.  In sample coordinates (gmp.hip:4-11: r = M-1-m, k = M-1-i,
// P_d[s] = |x[s]|^d, zero history)
//     j = m                         (j < 11)  : x[t-r]
//     j = 11 + (d * 11 + i) * 11 + m          : x[t-r] * P_{d+1}[t-r-k]
// so every operand element is ONE product of two LDS entries: a component of x (or of the target) and an envelope power (or 1).
// Staging converts the fp32 samples to fp64 and forms |x| = sqrt(I I + Q Q), |x|^2 .. |x|^4 in fp64 (repeated multiplication); the basis
// itself never exists in memory.
//
// Tiles: 496 = 31 tiles of 16 columns, in 8 blocks of 4 tiles (the last block's fourth tile is columns 496 .. 511: zero operands, never
// written).  The 36 block pairs (bi <= bj) of the upper triangle are the wave tasks: a wave keeps the 4 x 4 accumulator tiles of its pair
// (16 x 4 doubles per lane) and issues 16 MFMAs per K-step of four rows (two samples) from 8 operand values — lane (n = lane & 15,
// q = lane >> 4) of the operand of tile c holds A[row q][16 c + n], which is the A operand of the tiles (c, .) and the B operand of the
// tiles (., c) alike.  A workgroup = 4 waves = 4 block pairs on the same staged samples; 9 workgroups cover the triangle.
// Samples: items = (sequence, chunk of <= 512 samples), staged with the 20-sample look-back halo.  `slices` (<= 56) workgroup sets walk
// the items in a fixed interleave (slice s: items s, s + slices, ..) and keep their sums in registers; each slice writes ONE partial Gram
// (upper-triangle tiles) to the workspace, and a second kernel adds the slices in slice order and mirrors the triangle.  No atomics: the
// result depends on (B, T) alone, bit for bit.
#include "odpd_host.h"

namespace odpd {
namespace {

constexpr int kM = 11;                          // memory_length
constexpr int kHalo = 2 * (kM - 1);             // look-back of the oldest tap's envelope
constexpr int kCols = 496;                      // 495 basis columns + the target
constexpr int kBlocks = 8;                      // blocks of 4 tiles = 64 columns
constexpr int kPairs = kBlocks * (kBlocks + 1) / 2;
constexpr int kThreads = 256;
constexpr int kGroups = kPairs / 4;             // workgroups of a slice: four block pairs each
constexpr int kTC = 512;                        // samples of a chunk
constexpr int kMaxSlices = 56;                  // 9 x 56 workgroups: two per CU on 256 CUs
constexpr int kE = kTC + kHalo + 2;             // staged entries of an item (one past the end: the masked half of an odd tail)
// LDS planes of kE doubles: 0 Re x, 1 Im x, 2 Re target, 3 Im target, 4 zeros (columns 496 ..), 5 ones, 6 .. 9 |x|^1 .. |x|^4
constexpr int kPlanes = 10;
static_assert(kPairs % 4 == 0 && (kTC & 1) == 0, "four block pairs per workgroup; chunks start on a K-step");
static_assert(kPlanes * kE * sizeof(double) <= 64 * 1024, "static LDS");

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads, 2) void gmp_gram_kernel(const float2* __restrict__ x, const float2* __restrict__ tg, double* __restrict__ ws,
                                                               int T, int nchunk, int nitems, int slices) {
    __shared__ double sm[kPlanes * kE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, q = lane >> 4;
    const int slice = blockIdx.x / kGroups;
    int bi = 0, bj = (blockIdx.x % kGroups) * 4 + wave;              // block pair index -> (bi <= bj), row-major over the triangle
    while (bj >= kBlocks - bi) { bj -= kBlocks - bi; ++bi; }
    bj += bi;
    // operand u < 4: tile 4 bi + u; u >= 4: tile 4 bj + u - 4.  Row q of a K-step = sample q >> 1, part q & 1
    int ox[8], op[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int col = 64 * (u < 4 ? bi : bj) + 16 * (u & 3) + n;
        int xp = q & 1, pp = 5, r = 0, k = 0;
        if (col < kM) r = kM - 1 - col;
        else if (col < kCols - 1) {
            const int f = col - kM;
            pp = 6 + f / (kM * kM); k = kM - 1 - (f / kM) % kM; r = kM - 1 - f % kM;
        } else if (col == kCols - 1) xp += 2;
        else xp = 4;
        ox[u] = xp * kE + kHalo + (q >> 1) - r;
        op[u] = pp * kE + kHalo + (q >> 1) - r - k;
    }
    f64x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double tail = q < 2 ? 1.0 : 0.0;
    for (int item = slice; item < nitems; item += slices) {
        const int b = item / nchunk, t0 = (item - b * nchunk) * kTC;
        const int len = min(kTC, T - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < kE; e += kThreads) {
            const int t = t0 + e - kHalo;
            double xr = 0.0, xi = 0.0, tr = 0.0, ti = 0.0;
            if (t >= 0 && t < T) {                                   // zero history (gmp.py:26-27,33)
                const float2 v = x[(size_t)b * T + t];
                xr = (double)v.x; xi = (double)v.y;
                if (t >= t0 && t < t0 + len) { const float2 w = tg[(size_t)b * T + t]; tr = (double)w.x; ti = (double)w.y; }
            }
            const double a = sqrt(xr * xr + xi * xi), a2 = a * a;
            sm[e] = xr; sm[kE + e] = xi; sm[2 * kE + e] = tr; sm[3 * kE + e] = ti; sm[4 * kE + e] = 0.0; sm[5 * kE + e] = 1.0;
            sm[6 * kE + e] = a; sm[7 * kE + e] = a2; sm[8 * kE + e] = a2 * a; sm[9 * kE + e] = a2 * a2;
        }
        __syncthreads();
        const int nfull = len >> 1;
        for (int s = 0; s < nfull; ++s) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = sm[ox[u] + 2 * s] * sm[op[u] + 2 * s];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[i], v[4 + j], acc[i][j], 0, 0, 0);
        }
        if (len & 1) {                                               // the last sample alone: rows 2, 3 of the K-step are padding
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = sm[ox[u] + 2 * nfull] * sm[op[u] + 2 * nfull] * tail;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[i], v[4 + j], acc[i][j], 0, 0, 0);
        }
    }
    // f64 C/D map: acc[i][j][v] of lane (n, q) = D[row q + 4 v][col n] of tile (4 bi + i, 4 bj + j)
    double* out = ws + (size_t)slice * kCols * kCols;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * bi + i > 4 * bj + j) continue;                   // lower-triangle tiles of a diagonal block: never read
            const int col = 64 * bj + 16 * j + n;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 64 * bi + 16 * i + q + 4 * v;
                if (row < kCols && col < kCols) out[(size_t)row * kCols + col] = acc[i][j][v];
            }
        }
}

// gram[i][j] = gram[j][i] = sum over the slices, in slice order, of the upper-triangle element
__global__ __launch_bounds__(kThreads) void gmp_gram_reduce_kernel(const double* __restrict__ ws, double* __restrict__ gram, int slices) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= kCols * kCols) return;
    const int i = idx / kCols, j = idx - i * kCols;
    if (i > j) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += ws[(size_t)k * kCols * kCols + idx];
    gram[idx] = s;
    gram[(size_t)j * kCols + i] = s;
}

struct GramGeom { int nchunk, nitems, slices; };
GramGeom gram_geom(int B, int T) {
    GramGeom g;
    g.nchunk = (T + kTC - 1) / kTC;
    const int64_t items = (int64_t)B * g.nchunk;
    g.nitems = items > 0x7fffffff ? -1 : (int)items;
    // one slice per chunk's worth of samples (<= nitems: an item holds kTC samples at the most), so the workspace grows with B * T alone
    const int64_t full = ((int64_t)B * T + kTC - 1) / kTC;
    g.slices = full < kMaxSlices ? (int)full : kMaxSlices;
    return g;
}
// the float gmp model as the registry builds it: memory_length 11, no quantisation, no flags
int gram_model(const odpd_model_t* m) {
    if (!m) return ODPD_EINVAL;
    if (m->backbone != ODPD_GMP || m->hidden != kM || m->bits_w != 0 || m->bits_a != 0 || m->flags != 0) return ODPD_EUNSUPPORTED;
    return ODPD_OK;
}

}  // namespace
}  // namespace odpd

using namespace odpd;

extern "C" int64_t odpd_gmp_gram_workspace_bytes(const odpd_model_t* m, int B, int T) {
    if (const int e = gram_model(m)) return e;
    if (B <= 0 || T <= 0) return ODPD_EINVAL;
    const GramGeom g = gram_geom(B, T);
    if (g.nitems < 0) return ODPD_EINVAL;
    return (int64_t)g.slices * kCols * kCols * (int64_t)sizeof(double);
}

extern "C" int odpd_gmp_gram(void* stream, const odpd_model_t* m, const float* x, const float* target, int B, int T, double* gram,
                             void* workspace) {
    if (const int e = gram_model(m)) return e;
    if (!x || !target || !gram || !workspace || B <= 0 || T <= 0) return ODPD_EINVAL;
    const GramGeom g = gram_geom(B, T);
    if (g.nitems < 0) return ODPD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* ws = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(gmp_gram_kernel, dim3(g.slices * kGroups), dim3(kThreads), 0, st, reinterpret_cast<const float2*>(x),
                       reinterpret_cast<const float2*>(target), ws, T, g.nchunk, g.nitems, g.slices);
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(gmp_gram_reduce_kernel, dim3((kCols * kCols + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ws, gram, g.slices);
    return (int)hipGetLastError();
}
