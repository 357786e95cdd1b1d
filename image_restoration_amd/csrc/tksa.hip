// The c x c side of DRSformer's top-k sparse attention (TKSA, DRSformer_arch.py:101-171), c = C/heads <= 120, fp32 throughout.
// Everything outside the c x c matrices is MDTA's (modules.hip attn_core_fwd / attn_core_bwd): the pixel-axis Gram, the M_b
// GEMM and the dq / dk GEMMs.  What differs is the row map from S to A:
//   S = temperature * cos(q_i, k_j);  P_m = softmax over the k_m largest entries of each row of S (the rest -inf), m = 1..4;
//   A = sum_m w_m P_m   (w_m = attn1..attn4),  so  sum_m w_m (P_m v) = A v  and A folds into project_out as in MDTA.
// Ranks: entry j of row i is in mask m iff #{l : S_il > S_ij, or S_il == S_ij and l < j} < k_m (larger value first, then lower
// column index).  The backward recomputes the ranks, the row max, the exponentials and the four sums from the SAME saved S with the
// same code (tksa_row), so it uses exactly the forward's masks and probabilities.
// backward, with dA = W_o[:, head]^T dM[:, head]:
//   dS = sum_m w_m P_m (dA - rowdot(dA, P_m)),  d w_m = sum P_m dA  (per (image, head) partials, finished in a fixed order)
//   and from dS the temperature gradient and the [2c][2c] weights of the dq / dk GEMMs exactly as attn_small.hip builds them.
#include "internal.h"

namespace mi {

constexpr float TK_NORM_EPS = 1e-12f;   // F.normalize eps
constexpr int TKSA_MAX_C = 120;
constexpr int TK_KR = 16;               // rows of W_o / dM per staged chunk of the dA product

#define TKSA_CT_SWITCH(ct, CALL)                                       \
  do {                                                                 \
    switch (ct) {                                                      \
      case 1: { constexpr int CT = 1; CALL; } break;                   \
      case 2: { constexpr int CT = 2; CALL; } break;                   \
      case 3: { constexpr int CT = 3; CALL; } break;                   \
      case 4: { constexpr int CT = 4; CALL; } break;                   \
      case 5: case 6: { constexpr int CT = 6; CALL; } break;           \
      default: { constexpr int CT = 8; CALL; } break;                  \
    }                                                                  \
  } while (0)

// One matrix row per 16-lane DPP row: lane l16 holds columns l16 + 16 q.  Ss: S in LDS, row stride ld.  Returns the ranks, the
// exponentials e_q = exp(S - rowmax) (0 outside the c x c block) and the inverse sums of the four masked softmaxes.  Called under
// wave-uniform control flow (the DPP reductions need every lane).
template <int CT>
__device__ __forceinline__ void tksa_row(const float* Ss, int ld, int i, int c, int l16, const TopkArgs& tk, float (&sv)[CT],
                                         int (&rk)[CT], float (&e)[CT], float (&inv)[4]) {
  const bool rok = i < c;
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const int j = l16 + 16 * q;
    sv[q] = (rok && j < c) ? Ss[i * ld + j] : -INFINITY;
    mx = fmaxf(mx, sv[q]);
    rk[q] = 0;
  }
  if (rok) {
    for (int l = 0; l < c; ++l) {
      const float v = Ss[i * ld + l];
#pragma unroll
      for (int q = 0; q < CT; ++q) rk[q] += (v > sv[q] || (v == sv[q] && l < l16 + 16 * q)) ? 1 : 0;
    }
  }
  mx = row16_max(mx);
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const bool in = rok && l16 + 16 * q < c;
    e[q] = in ? expf(sv[q] - mx) : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) s4[m] += rk[q] < tk.k[m] ? e[q] : 0.f;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    s4[m] = row16_sum(s4[m]);
    inv[m] = rok ? 1.0f / s4[m] : 0.f;
  }
}

// forward, grid (Z): cosine P, S, ranks, the four softmaxes and A = sum_m w_m P_m of one (image, head).
template <int CT>
__global__ __launch_bounds__(256) void tksa_attn_kernel(const float* __restrict__ graw, const float* __restrict__ ss,
                                                        const float* __restrict__ temperature, TopkArgs tk, float* __restrict__ P,
                                                        float* __restrict__ S, float* __restrict__ A, float* __restrict__ nrm,
                                                        float* __restrict__ scores, int C, int heads) {
  constexpr int CP = 16 * CT;
  extern __shared__ float sm[];
  const int c = C / heads, ld = c + 1;
  float* Ss = sm;                 // [c][c + 1]
  float* inr = Ss + c * ld;       // [2 CP]
  const int z = blockIdx.x, h = z % heads;
  const int t = threadIdx.x, l16 = t & 15, g16 = t >> 4;
  const float* gz = graw + (int64_t)z * c * c;
  const float* sz = ss + (int64_t)z * 2 * c;
  for (int e = t; e < 2 * CP; e += 256) {
    const int k = e < CP ? e : e - CP;
    float v = 0.f;
    if (k < c) {
      const float n = fmaxf(sqrtf(sz[(e < CP ? 0 : c) + k]), TK_NORM_EPS);
      nrm[(int64_t)z * 2 * c + (e < CP ? 0 : c) + k] = n;
      v = 1.0f / n;
    }
    inr[e] = v;
  }
  __syncthreads();
  const float temp = temperature[h];
  const int64_t zo = (int64_t)z * c * c;
  for (int e = t; e < c * c; e += 256) {
    const int i = e / c, j = e - i * c;
    const float pv = gz[e] * inr[i] * inr[CP + j];
    const float s = pv * temp;
    P[zo + e] = pv;
    S[zo + e] = s;
    if (scores) scores[zo + e] = s;
    Ss[i * ld + j] = s;
  }
  __syncthreads();
  float w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) w[m] = tk.w[m][0];
#pragma unroll 1
  for (int it = 0; it < CT; ++it) {
    const int i = g16 + 16 * it;
    float sv[CT], e[CT], inv[4];
    int rk[CT];
    tksa_row<CT>(Ss, ld, i, c, l16, tk, sv, rk, e, inv);
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      float a = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) a += rk[q] < tk.k[m] ? w[m] * (e[q] * inv[m]) : 0.f;
      if (i < c && j < c) A[zo + i * c + j] = a;
    }
  }
}

// M[b][r][h c + j] = sum_i W_o[r][h c + i] A[b, h][i][j]  (+ bf16 copies of M_b and its transpose), grid (C/64, C/4, B)
__global__ __launch_bounds__(256) void tksa_fold_kernel(const float* __restrict__ A, const float* __restrict__ wo, float* __restrict__ M,
                                                        bf16* __restrict__ Mb, bf16* __restrict__ Mtb, int C, int heads) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (col >= C || r >= C) return;
  const int c = C / heads, h = col / c, j = col - h * c;
  const float* Az = A + (int64_t)(b * heads + h) * c * c + j;
  const float* wr = wo + (int64_t)r * C + h * c;
  float acc = 0.f;
  for (int i = 0; i < c; ++i) acc = fmaf(wr[i], Az[(int64_t)i * c], acc);
  const int64_t mb = (int64_t)b * C * C;
  M[mb + (int64_t)r * C + col] = acc;
  if (Mb) Mb[mb + (int64_t)r * C + col] = (bf16)acc;
  if (Mtb) Mtb[mb + (int64_t)col * C + r] = (bf16)acc;
}

// dWo_part[b][r][h c + i] = sum_j dM[b][r][h c + j] A[b, h][i][j], grid (C/64, C/4, B)
__global__ __launch_bounds__(256) void tksa_dwo_kernel(const float* __restrict__ dM, const float* __restrict__ A,
                                                       float* __restrict__ dwo_part, int C, int heads) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (col >= C || r >= C) return;
  const int c = C / heads, h = col / c, i = col - h * c;
  const float* dr = dM + (int64_t)b * C * C + (int64_t)r * C + h * c;
  const float* ai = A + (int64_t)(b * heads + h) * c * c + (int64_t)i * c;
  float acc = 0.f;
  for (int j = 0; j < c; ++j) acc = fmaf(dr[j], ai[j], acc);
  dwo_part[(int64_t)b * C * C + (int64_t)r * C + col] = acc;
}

static inline size_t tksa_bwd_lds_floats(int c, int ct) {
  const size_t cp = 16 * (size_t)ct;
  return (size_t)c * (c + 1) + 2 * TK_KR * cp + 16 * cp + cp + 16 * 4 + 4;
}

// backward of the c x c side, grid (Z): dA (fp32 FMA over the C rows of W_o and dM, staged through LDS), then per row the
// recomputed masks and softmaxes, dS, the d w_m / d temperature partials and the [2c][2c] dq / dk weights (attn_small.hip layout:
// rows 0..c-1 [G1 | D1], rows c..2c-1 [D2 | G1^T] over the stacked operand [k; q]).
template <int CT>
__global__ __launch_bounds__(256) void tksa_bwd_kernel(const float* __restrict__ dM, const float* __restrict__ S,
                                                       const float* __restrict__ P, const float* __restrict__ nrm,
                                                       const float* __restrict__ temperature, const float* __restrict__ wo,
                                                       TopkArgs tk, float* __restrict__ dtemp_part, float* __restrict__ dattn_part,
                                                       float* __restrict__ wd, bf16* __restrict__ wdb, int C, int heads) {
  constexpr int CP = 16 * CT;
  extern __shared__ float sm[];
  const int c = C / heads, ld = c + 1;
  float* Ss = sm;                        // [c][c + 1]
  float* Ws = Ss + c * ld;               // [KR][CP]
  float* Ds = Ws + TK_KR * CP;           // [KR][CP]
  float* colp = Ds + TK_KR * CP;         // [16][CP]
  float* rks = colp + 16 * CP;           // [CP]
  float* red = rks + CP;                 // [16][4] d w_m per row group, [4] d temperature per wave
  const int z = blockIdx.x, b = z / heads, h = z - b * heads;
  const int t = threadIdx.x, l16 = t & 15, g16 = t >> 4, lane = t & 63, wv = t >> 6;
  const int64_t zo = (int64_t)z * c * c;
  for (int e = t; e < c * c; e += 256) {
    const int i = e / c;
    Ss[i * ld + (e - i * c)] = S[zo + e];
  }
  // dA[i][j] = sum_r W_o[r][h c + i] dM[b][r][h c + j]; thread holds rows g16 + 16 it, columns l16 + 16 q
  float acc[CT][CT];
#pragma unroll
  for (int it = 0; it < CT; ++it)
#pragma unroll
    for (int q = 0; q < CT; ++q) acc[it][q] = 0.f;
  const float* dMb = dM + (int64_t)b * C * C + h * c;
  const float* wob = wo + h * c;
  for (int k0 = 0; k0 < C; k0 += TK_KR) {
    __syncthreads();
    for (int e = t; e < TK_KR * CP; e += 256) {
      const int rr = e / CP, j = e - rr * CP;
      const bool in = k0 + rr < C && j < c;
      Ws[e] = in ? wob[(int64_t)(k0 + rr) * C + j] : 0.f;
      Ds[e] = in ? dMb[(int64_t)(k0 + rr) * C + j] : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int rr = 0; rr < TK_KR; ++rr) {
      float wv_[CT], dv[CT];
#pragma unroll
      for (int it = 0; it < CT; ++it) wv_[it] = Ws[rr * CP + g16 + 16 * it];
#pragma unroll
      for (int q = 0; q < CT; ++q) dv[q] = Ds[rr * CP + l16 + 16 * q];
#pragma unroll
      for (int it = 0; it < CT; ++it)
#pragma unroll
        for (int q = 0; q < CT; ++q) acc[it][q] = fmaf(wv_[it], dv[q], acc[it][q]);
    }
  }
  __syncthreads();

  const float temp = temperature[h];
  float w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) w[m] = tk.w[m][0];
  const float* nz = nrm + (int64_t)z * 2 * c;
  float tsum = 0.f, dat[4] = {0.f, 0.f, 0.f, 0.f}, colsum[CT], rq[CT];
#pragma unroll
  for (int q = 0; q < CT; ++q) colsum[q] = 0.f;
#pragma unroll
  for (int it = 0; it < CT; ++it) {
    const int i = g16 + 16 * it;
    float sv[CT], e[CT], inv[4];
    int rk[CT];
    tksa_row<CT>(Ss, ld, i, c, l16, tk, sv, rk, e, inv);
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < CT; ++q)
#pragma unroll
      for (int m = 0; m < 4; ++m) dot[m] += rk[q] < tk.k[m] ? acc[it][q] * (e[q] * inv[m]) : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      dot[m] = row16_sum(dot[m]);
      dat[m] += dot[m];
    }
    float rqa = 0.f;
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      const bool in = i < c && j < c;
      float ds = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) ds += rk[q] < tk.k[m] ? w[m] * ((e[q] * inv[m]) * (acc[it][q] - dot[m])) : 0.f;
      ds = in ? ds : 0.f;
      const float pc = in ? P[zo + i * c + j] : 0.f;
      const float sp = in ? ds * sv[q] : 0.f;
      tsum += ds * pc;
      rqa += sp;
      colsum[q] += sp;
      acc[it][q] = ds;
    }
    rq[it] = row16_sum(rqa);
  }
#pragma unroll
  for (int q = 0; q < CT; ++q) colp[g16 * CP + l16 + 16 * q] = colsum[q];
  if (l16 == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) red[g16 * 4 + m] = dat[m];
  }
  tsum = wave_sum(tsum);
  if (lane == 0) red[64 + wv] = tsum;
  __syncthreads();
  if (t == 0) {
    dtemp_part[z] = (red[64] + red[65]) + (red[66] + red[67]);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float s = 0.f;
      for (int g = 0; g < 16; ++g) s += red[g * 4 + m];
      dattn_part[(int64_t)z * 4 + m] = s;
    }
  }
  for (int j = t; j < CP; j += 256) {
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s2 += colp[k * CP + j];
    rks[j] = s2;
  }
  __syncthreads();
  float* wq = wd + (int64_t)z * 2 * c * 2 * c;     // rows of dq
  float* wk = wq + (int64_t)c * 2 * c;            // rows of dk
  bf16* bq = wdb ? wdb + (int64_t)z * 2 * c * 2 * c : nullptr;
  bf16* bk = wdb ? bq + (int64_t)c * 2 * c : nullptr;
#pragma unroll
  for (int it = 0; it < CT; ++it) {
    const int i = g16 + 16 * it;
    if (i >= c) continue;
    const float nq = nz[i];
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      if (j >= c) continue;
      const float nk = nz[c + j];
      const float g1 = temp * acc[it][q] / (nq * nk);
      const bool dg = i == j;
      const float dq_ = (dg && nq > TK_NORM_EPS) ? -rq[it] / (nq * nq) : 0.f;
      const float dk_ = (dg && nk > TK_NORM_EPS) ? -rks[j] / (nk * nk) : 0.f;
      wq[i * 2 * c + j] = g1;              // dq_i += g1 k_j
      wq[i * 2 * c + c + j] = dq_;
      wk[i * 2 * c + j] = dk_;
      wk[j * 2 * c + c + i] = g1;          // dk_j += g1 q_i
      if (bq) {
        bq[i * 2 * c + j] = (bf16)g1; bq[i * 2 * c + c + j] = (bf16)dq_;
        bk[i * 2 * c + j] = (bf16)dk_; bk[j * 2 * c + c + i] = (bf16)g1;
      }
    }
  }
}

int tksa_check(int C, int heads, const int* k) {
  MI_CHECK_ARG(heads >= 1 && C >= 1 && C % heads == 0, "tksa: C=%d not divisible by heads=%d", C, heads);
  const int c = C / heads;
  MI_CHECK_ARG(c <= TKSA_MAX_C, "tksa: channels per head %d unsupported (1..%d)", c, TKSA_MAX_C);
  for (int m = 0; m < 4; ++m)
    MI_CHECK_ARG(k[m] >= 1 && k[m] <= c, "tksa: top-k size k%d=%d outside 1..c (c=%d)", m + 1, k[m], c);
  return MI_OK;
}

static inline int tksa_ct(int c) { return (c + 15) / 16; }

int launch_tksa_fold(const float* graw, const float* ss, const float* temperature, const TopkArgs& tk, const float* wo, float* P,
                     float* S, float* A, float* nrm, float* M, float* scores, int B, int C, int heads, hipStream_t st, void* Mb,
                     void* Mtb) {
  MI_TRY(tksa_check(C, heads, tk.k));
  MI_CHECK_ARG(graw && ss && temperature && wo && P && S && A && nrm && M, "tksa: null pointer in the attention fold");
  MI_CHECK_ARG(tk.w[0] && tk.w[1] && tk.w[2] && tk.w[3], "tksa: null attn1..4 pointer");
  const int c = C / heads, Z = B * heads;
  {
    ProfScope ps(st, K_TKSA_ATTN, 4.0 * Z * (5.0 * c * c + 2.0 * c), (double)Z * c * c * (c + 16.0));
    TKSA_CT_SWITCH(tksa_ct(c), {
      const size_t lds = ((size_t)c * (c + 1) + 2 * 16 * CT) * sizeof(float);
      if (lds > 64 * 1024)
        MI_CHECK_HIP(hipFuncSetAttribute((const void*)tksa_attn_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((tksa_attn_kernel<CT>), dim3(Z), dim3(256), lds, st, graw, ss, temperature, tk, P, S, A, nrm, scores, C,
                         heads);
    });
    MI_LAUNCH_CHECK();
  }
  ProfScope ps(st, K_TKSA_FOLD, 4.0 * B * (2.0 * C * C + (double)C * c), 2.0 * B * C * (double)c * C);
  hipLaunchKernelGGL(tksa_fold_kernel, dim3(cdiv(C, 64), cdiv(C, 4), B), dim3(256), 0, st, A, wo, M, (bf16*)Mb, (bf16*)Mtb, C, heads);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int launch_tksa_bwd(const float* dM, const float* A, const float* S, const float* P, const float* nrm, const float* temperature,
                    const TopkArgs& tk, const float* wo, float* dwo_part, float* dtemp_part, float* dattn_part, float* wd, int B,
                    int C, int heads, hipStream_t st, void* wdb) {
  MI_TRY(tksa_check(C, heads, tk.k));
  MI_CHECK_ARG(dM && A && S && P && nrm && temperature && wo && dwo_part && dtemp_part && dattn_part && wd,
               "tksa: null pointer in the attention backward");
  const int c = C / heads, Z = B * heads;
  {
    ProfScope ps(st, K_TKSA_BWD, 4.0 * B * (2.0 * C * C + 5.0 * heads * c * c), 2.0 * B * C * (double)c * C + (double)Z * c * c * c);
    TKSA_CT_SWITCH(tksa_ct(c), {
      const size_t lds = tksa_bwd_lds_floats(c, CT) * sizeof(float);
      if (lds > 64 * 1024)
        MI_CHECK_HIP(hipFuncSetAttribute((const void*)tksa_bwd_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((tksa_bwd_kernel<CT>), dim3(Z), dim3(256), lds, st, dM, S, P, nrm, temperature, wo, tk, dtemp_part,
                         dattn_part, wd, (bf16*)wdb, C, heads);
    });
    MI_LAUNCH_CHECK();
  }
  ProfScope ps(st, K_TKSA_DWO, 4.0 * B * (2.0 * C * C + (double)heads * c * c), 2.0 * B * C * (double)c * C);
  hipLaunchKernelGGL(tksa_dwo_kernel, dim3(cdiv(C, 64), cdiv(C, 4), B), dim3(256), 0, st, dM, A, dwo_part, C, heads);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // namespace mi
