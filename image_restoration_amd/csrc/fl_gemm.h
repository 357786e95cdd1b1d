// The dense-DFT GEMM shared by the FFT loss (fftloss.hip) and FreMLP / mi_dft2_* (fremlp.hip): complex C = A . B as chains of the
// exact fp32-input MFMA (v_mfma_f32_16x16x4_f32), the twiddle rule, and the tile-width rule.  Each translation unit gets its own
// copy (anonymous namespace) and instantiates only the prologue / epilogue modes it launches.
#pragma once
#include "internal.h"

namespace mi {
namespace {

constexpr int FL_MIN = 2, FL_MAX = 512;      // supported H and W
constexpr int FL_TM = 64;                    // rows per workgroup tile: four waves, one 16-row fragment each
constexpr int FL_KC = 16;                    // contraction depth per LDS stage (four k-steps of the 16x16x4 MFMA)
constexpr int FL_LDA = FL_KC + 1;            // A tile [64][17]: lane (row, k) -> 17 row + k, all 64 banks distinct
constexpr int FL_LDB = 80;                   // B tile [16][80]: 80 mod 64 = 16, so the four k rows of a fragment read land apart
constexpr int FL_THREADS = 256;

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

}  // namespace
}  // namespace mi
