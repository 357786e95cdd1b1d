// The real 2-D transforms rfft2 / irfft2 without an FFT library, the home of everything the FFT loss (fftloss.hip), FreMLP
// (fremlp.hip) and FourierUnit (sfh.hip) share (dft2.h): the dense-DFT GEMM, complex C = A . B as chains of the exact fp32-input
// MFMA (v_mfma_f32_16x16x4_f32); the twiddle rule and the one table fill; the tile-width rule and dft2_geom, the ONE place that
// decides tiles and grids; the stage launchers, the four directions built from them, the layout of the transform's own blob, and
// mi_dft2_workspace / mi_dft2_r2c / mi_dft2_c2r.  This is the only translation unit that instantiates fl_gemm_kernel.
#include <limits.h>

#include "dft2.h"

namespace mi {
namespace {

constexpr int FL_LDA = FL_KC + 1;            // A tile [64][17]: lane (row, k) -> 17 row + k, all 64 banks distinct
constexpr int FL_LDB = 80;                   // B tile [16][80]: 80 mod 64 = 16, so the four k rows of a fragment read land apart

// fragments per tile: the width that pads n the least (ties: the wider tile, fewer workgroups re-reading A)
inline int fl_pick_nf(int n) {
  int best = 5, best_pad = cdiv(n, 80) * 80;
  for (int nf = 4; nf >= 3; --nf) {
    const int pad = cdiv(n, 16 * nf) * 16 * nf;
    if (pad < best_pad) { best = nf; best_pad = pad; }
  }
  return best;
}

// cos and sin of 2 pi r / N for 0 <= r < N.  The angle is folded into the first quadrant in integers, so the argument of
// sincospif is m / N with 0 <= m <= N / 2 and every multiple of a quarter turn comes out exactly 0 or +-1.
__device__ __forceinline__ void fl_twiddle(int r, int N, float* c, float* s) {
  float ss = 1.f, cs = 1.f;
  if (2 * r > N) { r = N - r; ss = -1.f; }        // theta -> 2 pi - theta
  int m = 2 * r;                                   // theta = pi m / N, 0 <= m <= N
  if (2 * m > N) { m = N - m; cs = -1.f; }        // theta -> pi - theta
  float sv, cv;
  sincospif((float)m / (float)N, &sv, &cv);
  *c = cs * cv; *s = ss * sv;
}

// t: the DT_* tables.  The four weighted ones are filled where given (all four or none).
struct FlTables { float* t[DFT2_TABLES]; };
__global__ __launch_bounds__(FL_THREADS) void fl_tables_kernel(const FlTables tb, int H, int W, int K) {
  const int idx = blockIdx.x * FL_THREADS + threadIdx.x;
  float c, s;
  if (idx < W * K) {
    const int x = idx / K, l = idx - x * K;
    fl_twiddle((x * l) % W, W, &c, &s);
    tb.t[DT_CW][idx] = c; tb.t[DT_SW][idx] = s;
    tb.t[DT_CWT][l * W + x] = c; tb.t[DT_SWT][l * W + x] = s;
    if (tb.t[DT_WCW]) {
      const float wl = (l == 0 || 2 * l == W) ? 1.f : 2.f;      // odd W has no Nyquist column
      tb.t[DT_WCW][idx] = wl * c; tb.t[DT_WSW][idx] = wl * s;
      tb.t[DT_WCWT][l * W + x] = wl * c; tb.t[DT_WSWT][l * W + x] = wl * s;
    }
  } else if (idx < W * K + H * H) {
    const int j = idx - W * K;
    const int k = j / H, y = j - k * H;
    fl_twiddle((k * y) % H, H, &c, &s);
    tb.t[DT_CH][j] = c; tb.t[DT_SH][j] = s;
  }
}

struct FlGemm {
  const void* a0; const void* a1;     // A re / im, fp32 [M][lda] (+ z a_zs);  A_DIFF: pred / target in the activation dtype;
                                      // A_REAL: a0 alone, in the activation dtype
  const float* b0; const float* b1;   // B re / im, fp32 [Kd][ldb] (+ z b_zs)
  void* c0; float* c1;                // out re / im [M][ldc] (+ z c_zs);  E_REAL: c0 in the activation dtype, c1 unused
  float* part;                        // E_SIGN: one |re| + |im| sum per workgroup
  int64_t a_zs, b_zs, c_zs;
  int lda, ldb, ldc;
  int M, N, Kd;
  int m_tiles, n_tiles;
  float a_sign, b_sign, scale;        // factors (+-1) on the imaginary operands as they are staged; E_REAL: output scale
};
enum { A_DIFF = 0, A_CPLX = 1, A_REAL = 2 };      // A = pred - target (real) / a complex fp32 matrix / one real tensor
enum { E_CPLX = 0, E_SIGN = 1, E_REAL = 2 };      // store re and im / store their signs and sum |.| / store scale * re only

// C = A . B over complex operands: Cre = Are Bre - Aim Bim, Cim = Are Bim + Aim Bre, each product a chain of 16x16x4 fp32 MFMAs.
// A workgroup owns a 64 x (16 NF) tile; wave w owns its rows 16 w .. 16 w + 15.  Operands are staged through LDS 16 k at a time,
// zero-padded at every edge (rows past M, columns past N, k past Kd), and the next stage's global loads are issued before the
// current stage's MFMAs.  Nothing outside [M][Kd], [Kd][N] and [M][N] is read or written.
template <int AM, int EM, typename T, int NF>
__global__ __launch_bounds__(FL_THREADS) void fl_gemm_kernel(const FlGemm g) {
  constexpr int TN = 16 * NF;
  __shared__ float sA[2][FL_TM * FL_LDA];
  __shared__ float sB[2][FL_KC * FL_LDB];
  __shared__ float sred[FL_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bid = blockIdx.x;
  const int nt = bid % g.n_tiles; bid /= g.n_tiles;
  const int mt = bid % g.m_tiles;
  const int64_t z = bid / g.m_tiles;
  const int m0 = mt * FL_TM, n0 = nt * TN;
  const T* at0 = (const T*)g.a0; const T* at1 = (const T*)g.a1;                      // A_DIFF, A_REAL
  const float* af0 = (const float*)g.a0 + z * g.a_zs; const float* af1 = (const float*)g.a1 + z * g.a_zs;   // A_CPLX
  const float* b0 = g.b0 + z * g.b_zs; const float* b1 = g.b1 + z * g.b_zs;

  float ra[2][4], rb[2][NF];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + FL_THREADS * i;
      const int row = m0 + (e >> 4), k = k0 + (e & 15);
      const bool ok = row < g.M && k < g.Kd;
      const int64_t o = (int64_t)row * g.lda + k;
      if (AM == A_DIFF) {
        ra[0][i] = ok ? ld1(at0 + o) - ld1(at1 + o) : 0.f;
        ra[1][i] = 0.f;
      } else if (AM == A_REAL) {
        ra[0][i] = ok ? ld1(at0 + o) : 0.f;
        ra[1][i] = 0.f;
      } else {
        ra[0][i] = ok ? af0[o] : 0.f;
        ra[1][i] = ok ? g.a_sign * af1[o] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int e = tid + FL_THREADS * i;
      const int kk = e / TN, n = n0 + (e - kk * TN), k = k0 + kk;
      const bool ok = k < g.Kd && n < g.N;
      const int64_t o = (int64_t)k * g.ldb + n;
      rb[0][i] = ok ? b0[o] : 0.f;
      rb[1][i] = ok ? g.b_sign * b1[o] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + FL_THREADS * i;
      const int o = (e >> 4) * FL_LDA + (e & 15);
      sA[0][o] = ra[0][i];
      if (AM == A_CPLX) sA[1][o] = ra[1][i];
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int e = tid + FL_THREADS * i;
      const int kk = e / TN;
      const int o = kk * FL_LDB + (e - kk * TN);
      sB[0][o] = rb[0][i];
      sB[1][o] = rb[1][i];
    }
  };

  f32x4 cr[NF], ci[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) { cr[f] = f32x4{0.f, 0.f, 0.f, 0.f}; ci[f] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  // operand lane maps of v_mfma_f32_16x16x4_f32: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]
  const int a_off = (wave * 16 + (lane & 15)) * FL_LDA + (lane >> 4);
  const int b_off = (lane >> 4) * FL_LDB + (lane & 15);
  load(0);
  for (int k0 = 0; k0 < g.Kd; k0 += FL_KC) {
    __syncthreads();                       // the previous stage's fragment reads are done
    stage();
    __syncthreads();
    if (k0 + FL_KC < g.Kd) load(k0 + FL_KC);
#pragma unroll
    for (int ks = 0; ks < FL_KC / 4; ++ks) {
      const float ar = sA[0][a_off + 4 * ks];
      float ai = 0.f, nai = 0.f;
      if (AM == A_CPLX) { ai = sA[1][a_off + 4 * ks]; nai = -ai; }
      float br[NF], bi[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        br[f] = sB[0][b_off + 4 * ks * FL_LDB + 16 * f];
        bi[f] = sB[1][b_off + 4 * ks * FL_LDB + 16 * f];
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) cr[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br[f], cr[f], 0, 0, 0);
      if (EM != E_REAL) {
#pragma unroll
        for (int f = 0; f < NF; ++f) ci[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi[f], ci[f], 0, 0, 0);
      }
      if (AM == A_CPLX) {
#pragma unroll
        for (int f = 0; f < NF; ++f) cr[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(nai, bi[f], cr[f], 0, 0, 0);
        if (EM != E_REAL) {
#pragma unroll
          for (int f = 0; f < NF; ++f) ci[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[f], ci[f], 0, 0, 0);
        }
      }
    }
  }

  // C/D map: col = lane & 15, row = 4 (lane >> 4) + register
  float asum = 0.f;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int n = n0 + 16 * f + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 16 + 4 * (lane >> 4) + r;
      if (m >= g.M || n >= g.N) continue;
      const int64_t o = z * g.c_zs + (int64_t)m * g.ldc + n;
      const float vr = cr[f][r], vi = ci[f][r];
      if (EM == E_CPLX) {
        ((float*)g.c0)[o] = vr;
        g.c1[o] = vi;
      } else if (EM == E_SIGN) {
        asum += fabsf(vr) + fabsf(vi);
        if (g.c0) {                                                   // sign(0) = 0, of either zero
          ((float*)g.c0)[o] = (float)((vr > 0.f) - (vr < 0.f));
          g.c1[o] = (float)((vi > 0.f) - (vi < 0.f));
        }
      } else {
        st1((T*)g.c0 + o, g.scale * vr);
      }
    }
  }
  if (EM == E_SIGN) {            // lanes, then waves, in a fixed order
    asum = wave_sum(asum);
    if (lane == 0) sred[wave] = asum;
    __syncthreads();
    if (tid == 0) g.part[blockIdx.x] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
  }
}

template <int AM, int EM, typename T>
int fl_launch(int nf, const FlGemm& g, int grid, hipStream_t st) {
  if (nf == 3) hipLaunchKernelGGL((fl_gemm_kernel<AM, EM, T, 3>), dim3(grid), dim3(FL_THREADS), 0, st, g);
  else if (nf == 4) hipLaunchKernelGGL((fl_gemm_kernel<AM, EM, T, 4>), dim3(grid), dim3(FL_THREADS), 0, st, g);
  else hipLaunchKernelGGL((fl_gemm_kernel<AM, EM, T, 5>), dim3(grid), dim3(FL_THREADS), 0, st, g);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

// the per-plane columns stage: (cos H + i sign sin H) . in, one set of tiles per plane
FlGemm fl_cols(const Dft2Geom& p, const Dft2Ws& w, float sign, const float* ire, const float* iim, float* ore, float* oim) {
  const int64_t plane = (int64_t)p.H * p.K;
  FlGemm g = {};
  g.a0 = w.tab[DT_CH]; g.a1 = w.tab[DT_SH]; g.lda = p.H; g.a_sign = sign;
  g.b0 = ire; g.b1 = iim; g.ldb = p.K; g.b_zs = plane; g.b_sign = 1.f;
  g.c0 = ore; g.c1 = oim; g.ldc = p.K; g.c_zs = plane;
  g.M = p.H; g.N = p.K; g.Kd = p.H; g.m_tiles = p.m_tiles_plane; g.n_tiles = p.l_blocks;
  return g;
}

int dft2_check(const char* who, int B, int C, int H, int W, int dtype, Dft2Geom* g, Dft2Blob* b) {
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "%s: bad dtype %d", who, dtype);
  MI_CHECK_ARG(B > 0 && C > 0, "%s: bad shape B=%d C=%d", who, B, C);
  MI_CHECK_ARG(H >= FL_MIN && W >= FL_MIN && H <= FL_MAX && W <= FL_MAX,
               "%s: H=%d W=%d outside the supported %d..%d (there is no fallback)", who, H, W, FL_MIN, FL_MAX);
  MI_CHECK_ARG(dft2_geom((int64_t)B * C, H, W, g) && dft2_blob(*g, b), "%s: too many planes (B=%d C=%d H=%d)", who, B, C, H);
  return MI_OK;
}

}  // namespace

bool dft2_geom(int64_t P, int H, int W, Dft2Geom* p) {
  *p = Dft2Geom{};
  if (P <= 0 || H < FL_MIN || W < FL_MIN || H > FL_MAX || W > FL_MAX) return false;
  if (P * H > (1 << 30)) return false;
  const int K = W / 2 + 1;
  const int nf_l = fl_pick_nf(K), nf_x = fl_pick_nf(W);
  const int l_blocks = cdiv(K, 16 * nf_l), x_blocks = cdiv(W, 16 * nf_x);
  const int m_tiles_fold = cdiv(P * H, FL_TM), m_tiles_plane = cdiv(H, FL_TM);
  const int64_t g1 = (int64_t)m_tiles_fold * l_blocks, g2 = P * m_tiles_plane * l_blocks, g4 = (int64_t)m_tiles_fold * x_blocks;
  if (g1 > INT_MAX || g2 > INT_MAX || g4 > INT_MAX) return false;
  p->P = (int)P; p->H = H; p->W = W; p->K = K;
  p->nf_l = nf_l; p->nf_x = nf_x; p->l_blocks = l_blocks; p->x_blocks = x_blocks;
  p->m_tiles_fold = m_tiles_fold; p->m_tiles_plane = m_tiles_plane;
  p->grid_tab = cdiv((int64_t)W * K + (int64_t)H * H, FL_THREADS);
  p->grid_fold_l = (int)g1; p->grid_plane = (int)g2; p->grid_fold_x = (int)g4;
  return true;
}

bool dft2_blob(const Dft2Geom& g, Dft2Blob* b) {
  *b = Dft2Blob{};
  const int64_t bins = (int64_t)g.P * g.H * g.K;
  if (bins > INT_MAX) return false;
  size_t o = 0;
  for (int i = 0; i < DFT2_TABLES; ++i) { b->tab[i] = o; o = align_up(o + dft2_table_bytes(g, i), 256); }
  b->t = o; b->bins = bins;
  b->total = align_up(o + (size_t)bins * 2 * 4, 256);
  return true;
}

Dft2Ws dft2_blob_ws(const Dft2Blob& b, void* base) {
  Dft2Ws w;
  for (int i = 0; i < DFT2_TABLES; ++i) w.tab[i] = (float*)((char*)base + b.tab[i]);
  w.tre = (float*)((char*)base + b.t); w.tim = w.tre + b.bins;
  return w;
}

int dft2_tables(const Dft2Geom& g, const Dft2Ws& w, hipStream_t st) {
  FlTables tb;
  for (int i = 0; i < DFT2_TABLES; ++i) tb.t[i] = w.tab[i];
  hipLaunchKernelGGL(fl_tables_kernel, dim3(g.grid_tab), dim3(FL_THREADS), 0, st, tb, g.H, g.W, g.K);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int dft2_rows_fwd(const Dft2Geom& p, const void* x, const void* sub, const float* tc, const float* ts, float* ore, float* oim, int dtype,
                  hipStream_t st) {
  FlGemm g = {};
  g.a0 = x; g.a1 = sub; g.lda = p.W;
  g.b0 = tc; g.b1 = ts; g.ldb = p.K; g.b_sign = -1.f;
  g.c0 = ore; g.c1 = oim; g.ldc = p.K;
  g.M = p.P * p.H; g.N = p.K; g.Kd = p.W; g.m_tiles = p.m_tiles_fold; g.n_tiles = p.l_blocks;
  return with_dtype(dtype, "dft2_rows_fwd", [&](auto tag) -> int {
    return sub ? fl_launch<A_DIFF, E_CPLX, decltype(tag)>(p.nf_l, g, p.grid_fold_l, st)
               : fl_launch<A_REAL, E_CPLX, decltype(tag)>(p.nf_l, g, p.grid_fold_l, st);
  });
}

int dft2_cols(const Dft2Geom& p, const Dft2Ws& w, float sign, const float* ire, const float* iim, float* ore, float* oim, hipStream_t st) {
  return fl_launch<A_CPLX, E_CPLX, float>(p.nf_l, fl_cols(p, w, sign, ire, iim, ore, oim), p.grid_plane, st);
}

int dft2_cols_sign(const Dft2Geom& p, const Dft2Ws& w, const float* ire, const float* iim, float* sre, float* sim, float* part,
                   hipStream_t st) {
  FlGemm g = fl_cols(p, w, -1.f, ire, iim, sre, sim);
  g.part = part;
  return fl_launch<A_CPLX, E_SIGN, float>(p.nf_l, g, p.grid_plane, st);
}

int dft2_rows_bwd(const Dft2Geom& p, const float* ire, const float* iim, const float* tc, const float* ts, void* out, float scale,
                  int dtype, hipStream_t st) {
  FlGemm g = {};
  g.a0 = ire; g.a1 = iim; g.lda = p.K; g.a_sign = 1.f;
  g.b0 = tc; g.b1 = ts; g.ldb = p.W; g.b_sign = 1.f;
  g.c0 = out; g.ldc = p.W; g.scale = scale;
  g.M = p.P * p.H; g.N = p.W; g.Kd = p.K; g.m_tiles = p.m_tiles_fold; g.n_tiles = p.x_blocks;
  return with_dtype(dtype, "dft2_rows_bwd", [&](auto tag) -> int {
    return fl_launch<A_CPLX, E_REAL, decltype(tag)>(p.nf_x, g, p.grid_fold_x, st);
  });
}

int dft2_r2c_run(const Dft2Geom& g, const Dft2Ws& w, const void* x, float* zre, float* zim, int dtype, hipStream_t st) {
  MI_TRY(dft2_rows_fwd(g, x, nullptr, w.tab[DT_CW], w.tab[DT_SW], w.tre, w.tim, dtype, st));
  return dft2_cols(g, w, -1.f, w.tre, w.tim, zre, zim, st);
}
int dft2_c2r_run(const Dft2Geom& g, const Dft2Ws& w, const float* yre, const float* yim, void* out, int dtype, hipStream_t st) {
  MI_TRY(dft2_cols(g, w, 1.f, yre, yim, w.tre, w.tim, st));
  return dft2_rows_bwd(g, w.tre, w.tim, w.tab[DT_WCWT], w.tab[DT_WSWT], out, (float)(1.0 / ((double)g.H * g.W)), dtype, st);
}
int dft2_c2r_adj(const Dft2Geom& g, const Dft2Ws& w, const void* dout, float* gre, float* gim, int dtype, hipStream_t st) {
  MI_TRY(dft2_rows_fwd(g, dout, nullptr, w.tab[DT_WCW], w.tab[DT_WSW], w.tre, w.tim, dtype, st));
  return dft2_cols(g, w, -1.f, w.tre, w.tim, gre, gim, st);
}
int dft2_r2c_adj(const Dft2Geom& g, const Dft2Ws& w, const float* dre, const float* dim, void* dx, int dtype, hipStream_t st) {
  MI_TRY(dft2_cols(g, w, 1.f, dre, dim, w.tre, w.tim, st));
  return dft2_rows_bwd(g, w.tre, w.tim, w.tab[DT_CWT], w.tab[DT_SWT], dx, 1.f, dtype, st);
}
}  // namespace mi

using namespace mi;

extern "C" size_t mi_dft2_workspace(int B, int C, int H, int W) {
  Dft2Geom g; Dft2Blob b;
  return B > 0 && C > 0 && dft2_geom((int64_t)B * C, H, W, &g) && dft2_blob(g, &b) ? b.total : 0;
}

extern "C" int mi_dft2_r2c(const void* x, float* zre, float* zim, int B, int C, int H, int W, int dtype, void* ws, void* stream) {
  MI_CHECK_ARG(x && zre && zim && ws, "dft2_r2c: null pointer");
  Dft2Geom g; Dft2Blob b;
  MI_TRY(dft2_check("dft2_r2c", B, C, H, W, dtype, &g, &b));
  const Dft2Ws w = dft2_blob_ws(b, ws);
  MI_TRY(dft2_tables(g, w, (hipStream_t)stream));
  return dft2_r2c_run(g, w, x, zre, zim, dtype, (hipStream_t)stream);
}

extern "C" int mi_dft2_c2r(const float* yre, const float* yim, void* out, int B, int C, int H, int W, int dtype, void* ws,
                           void* stream) {
  MI_CHECK_ARG(yre && yim && out && ws, "dft2_c2r: null pointer");
  Dft2Geom g; Dft2Blob b;
  MI_TRY(dft2_check("dft2_c2r", B, C, H, W, dtype, &g, &b));
  const Dft2Ws w = dft2_blob_ws(b, ws);
  MI_TRY(dft2_tables(g, w, (hipStream_t)stream));
  return dft2_c2r_run(g, w, yre, yim, out, dtype, (hipStream_t)stream);
}
