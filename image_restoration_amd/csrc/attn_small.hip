// The c x c side of MDTA (c = C/heads <= 120): everything that happens between the long pixel-axis
// contractions (Restormer.py:121-127).  One workgroup per (image, head); fp32 throughout.
//
// forward  : cosine P = (q k^T)/(|q||k|), S = temperature*P, A = softmax_row(S), and the fold
//            M_b[:, head cols] = W_o[:, head cols] * A   so that  project_out(attn @ v) == M_b @ v
//            (one 1x1 GEMM per image instead of attn@v followed by project_out).
// backward : from dM_b = dY V^T:  dW_o, dA, dS (softmax bwd), d temperature, and the small matrices
//            that turn the gradients of the L2-normalised q,k into two more per-image 1x1 GEMMs:
//              dq = G1 k + diag(D1) q,  dk = G1^T q + diag(D2) k
//            with G1 = temperature*dS/(|q_i||k_j|), D1_i = -sum_j dS_ij S_ij/|q_i|^2, D2_j likewise.
#include "internal.h"

namespace mi {

constexpr float NORM_EPS = 1e-12f;  // F.normalize eps (Restormer.py:121-122)
constexpr int ATTN_MAX_C = 128;     // 16x16 threads x (up to) 8x8 register tile
constexpr int ATT_RC = 16;          // rows of W_o / dM handled by one workgroup

static inline int attn_ct(int c) { return (c + 15) / 16; }
static inline int attn_rchunks(int C) { return (C + ATT_RC - 1) / ATT_RC; }

// LDS floats of attn_fold_kernel<CT> with rpw row chunks of W_o per workgroup
static inline size_t attn_fold_lds_floats(int ct, int rpw) {
  const size_t cp = 16 * (size_t)ct;
  return cp * (cp + 1) + 2 * cp + (size_t)rpw * ATT_RC * (cp + 1);
}

// forward: grid (Z, ceil(C/16 / rpw)).  Every workgroup redoes the c x c cosine / temperature / row softmax of its (image, head)
// and folds rpw chunks of 16 rows of W_o:  M[b][r][h*c+j] = sum_i W_o[r][h*c+i] A[i][j].  The workgroups of row group 0 also
// store P, A and the norms.
//  * softmax: a 16-lane DPP row owns a matrix row (lane l16 holds columns l16 + 16 q), 16 matrix rows per pass, CT passes; all
//    global loads are issued up front, max / sum are 4-step DPP all-reduces, the 2c inverse norms come from LDS.  (The first
//    form - one wave per row, integer divisions to find (i, j), three sqrt / div per element - took 29 us at c = 96 and 57 us
//    at C = 384 where 24 row chunks each redid it: profiles/r04_f_attn_small.txt.)
//  * fold: fp32 MFMA (16x16x4): a wave owns 16 x 16 output tiles, both operands read from LDS one float per lane and step.
template <int CT>
__global__ __launch_bounds__(256) void attn_fold_kernel(const float* __restrict__ graw, const float* __restrict__ ss,
                                                        const float* __restrict__ temperature, const float* __restrict__ wo,
                                                        float* __restrict__ P, float* __restrict__ A, float* __restrict__ nrm,
                                                        float* __restrict__ M, bf16* __restrict__ Mb, bf16* __restrict__ Mtb, int C,
                                                        int heads, int rpw, int tb_vec) {
  constexpr int CP = 16 * CT, LD = CP + 1;
  extern __shared__ float sm[];
  float* As = sm;                       // [CP][LD]; rows and columns >= c are zero
  float* inr = As + CP * LD;            // [2 CP] 1 / max(|q_i|, eps), 1 / max(|k_j|, eps)
  float* Wt = inr + 2 * CP;             // [rpw * 16][LD]; columns >= c and rows >= C are zero
  const int c = C / heads;
  const int z = blockIdx.x, b = z / heads, h = z - b * heads;
  const int rch = (C + ATT_RC - 1) / ATT_RC;
  const int rc0 = blockIdx.y * rpw;
  const int nrc = rch - rc0 < rpw ? rch - rc0 : rpw;     // row chunks of this workgroup
  const int t = threadIdx.x, l16 = t & 15, g16 = t >> 4;
  const bool first = blockIdx.y == 0;
  const float* gz = graw + (int64_t)z * c * c;
  const float* sz = ss + (int64_t)z * 2 * c;

  float gv[CT][CT];
#pragma unroll
  for (int it = 0; it < CT; ++it) {
    const int i = g16 + 16 * it;
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      gv[it][q] = (i < c && j < c) ? gz[i * c + j] : 0.f;
    }
  }
  for (int e = t; e < nrc * ATT_RC * CP; e += 256) {
    const int rr = e / CP, col = e - rr * CP, r = rc0 * ATT_RC + rr;
    Wt[rr * LD + col] = (r < C && col < c) ? wo[(int64_t)r * C + h * c + col] : 0.f;
  }
  for (int e = t; e < 2 * CP; e += 256) {
    const int k = e < CP ? e : e - CP;
    float v = 0.f;
    if (k < c) {
      const float n = fmaxf(sqrtf(sz[(e < CP ? 0 : c) + k]), NORM_EPS);
      if (first) nrm[(int64_t)z * 2 * c + (e < CP ? 0 : c) + k] = n;
      v = 1.0f / n;
    }
    inr[e] = v;
  }
  __syncthreads();
  const float temp = temperature[h];
  float* Pz = P + (int64_t)z * c * c;
  float* Az = A + (int64_t)z * c * c;
#pragma unroll
  for (int it = 0; it < CT; ++it) {
    const int i = g16 + 16 * it;
    const bool rok = i < c;
    const float iq = inr[i];
    float sv[CT], mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      const float pv = gv[it][q] * iq * inr[CP + j];
      if (first && rok && j < c) Pz[i * c + j] = pv;
      sv[q] = (j < c || !rok) ? pv * temp : -INFINITY;     // (padding rows: all zeros, kept finite)
      mx = fmaxf(mx, sv[q]);
    }
    mx = row16_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < CT; ++q) { sv[q] = expf(sv[q] - mx); sum += sv[q]; }
    sum = row16_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int j = l16 + 16 * q;
      const bool in = rok && j < c;
      const float av = in ? sv[q] * inv : 0.f;
      As[i * LD + j] = av;
      if (first && in) Az[i * c + j] = av;
    }
  }
  __syncthreads();

  const int wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, li = lane & 15, kq = lane >> 4;
  for (int tile = wv; tile < nrc * CT; tile += 4) {
    const int rr = tile / CT, nt = tile - rr * CT;
    const float* wp = Wt + (rr * ATT_RC + li) * LD + kq;
    const float* ap = As + kq * LD + 16 * nt + li;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < CP / 4; ++ks) d = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[4 * ks], ap[4 * ks * LD], d, 0, 0, 0);
    // lane holds M[r .. r + 3][h c + j],  r = 16 (rc0 + rr) + 4 kq,  j = 16 nt + li
    const int r = (rc0 + rr) * ATT_RC + 4 * kq, j = 16 * nt + li;
    if (j < c) {
      const int64_t mb = (int64_t)b * C * C;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (r + i < C) {
          M[mb + (int64_t)(r + i) * C + h * c + j] = d[i];
          // bf16 copies for the per-image-weight GEMMs (mi_pw_desc.w_b16): M_b for out = M_b v, its transpose for dv = M_b^T dy
          if (Mb) Mb[mb + (int64_t)(r + i) * C + h * c + j] = (bf16)d[i];
        }
      if (Mtb) {
        bf16* tp = Mtb + mb + (int64_t)(h * c + j) * C + r;
        if (tb_vec && r + 3 < C) {
          *reinterpret_cast<u32x2*>(tp) = (u32x2){cvt_pk_bf16(d[0], d[1]), cvt_pk_bf16(d[2], d[3])};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (r + i < C) tp[i] = (bf16)d[i];
        }
      }
    }
  }
}

// backward of the c x c side, one launch: grid (Z, 1 + ceil(C / 64)).
//  y == 0: dA = W_o[:, head]^T dM[:, head] over all C rows (fp32 MFMA, both operands staged through LDS in chunks of 32 rows), then in
//          registers: softmax backward dS = A (dA - rowdot), d temperature, and the per-image weights of the gradient GEMM(s)
//          dq = G1 k + D1 q,  dk = G1^T q + D2 k  with G1 = temperature dS/(|q_i||k_j|), D1_i = -sum_j dS_ij S_ij/|q_i|^2,
//          D2_j = -sum_i dS_ij S_ij/|k_j|^2, as ONE [2c][2c] matrix per (image, head) acting on the stacked operand [k; q]:
//            rows 0..c-1  (dq): [ G1    | D1 ]        rows c..2c-1 (dk): [ D2 | G1^T ]
//          so that both gradients come out of one pass over q and k (mi_pw_desc.y_split), or of two GEMMs over row halves.
//          Wave w owns the row blocks mt = w, w + 4 of dA (all their column tiles): row sums are 16-lane DPP all-reduces.
//  y >= 1: 64 rows of dW_o:  dWo_part[b][r][h*c+i] = sum_j dM[r][h*c+j] A[i][j]   (fp32 MFMA, 16 rows per wave).
// (The first form - a partial kernel per 16-row chunk writing c x c partials of dA, CT x CT outer products on the VALU, and a
//  finishing kernel summing them - took 65 us at c = 96 and 67 us at C = 384: profiles/r04_f_attn_small.txt.)
constexpr int ATT_KR = 32;    // rows of W_o / dM per staged chunk (y == 0)
constexpr int ATT_RW = 64;    // rows of dW_o per workgroup (y >= 1)
static inline size_t attn_bwd_lds_floats(int ct) {
  const size_t cp = 16 * (size_t)ct, ld = cp + 1;
  const size_t r0 = 2 * ATT_KR * ld + 16 * cp + 2 * cp + 8, r1 = cp * ld + ATT_RW * ld;
  return r0 > r1 ? r0 : r1;
}
template <int CT>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ dM, const float* __restrict__ A,
                                                       const float* __restrict__ P, const float* __restrict__ nrm,
                                                       const float* __restrict__ temperature, const float* __restrict__ wo,
                                                       float* __restrict__ dwo_part, float* __restrict__ dtemp_part,
                                                       float* __restrict__ wd, bf16* __restrict__ wdb, int C, int heads, int vec) {
  constexpr int CP = 16 * CT, LD = CP + 1, MB = (CT + 3) / 4;
  extern __shared__ float sm[];
  const int c = C / heads;
  const int z = blockIdx.x, b = z / heads, h = z - b * heads;
  const int t = threadIdx.x, lane = t & 63, li = lane & 15, kq = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const float* dMb = dM + (int64_t)b * C * C + h * c;      // column block of this head
  const float* Az = A + (int64_t)z * c * c;

  if (blockIdx.y > 0) {
    // ---- rows of dW_o
    float* As = sm;                 // [CP][LD]  A, zero padded
    float* Ds = As + CP * LD;       // [RW][LD]  dM rows, zero padded
    const int r0 = (blockIdx.y - 1) * ATT_RW;
    for (int e = t; e < CP * CP; e += 256) {
      const int i = e / CP, j = e - i * CP;
      As[i * LD + j] = (i < c && j < c) ? Az[i * c + j] : 0.f;
    }
    for (int e = t; e < ATT_RW * CP; e += 256) {
      const int rr = e / CP, j = e - rr * CP;
      Ds[rr * LD + j] = (r0 + rr < C && j < c) ? dMb[(int64_t)(r0 + rr) * C + j] : 0.f;
    }
    __syncthreads();
    if (r0 + 16 * wv >= C) return;
    const float* dp = Ds + (16 * wv + li) * LD + kq;
    f32x4 d[CT];
#pragma unroll
    for (int nt = 0; nt < CT; ++nt) d[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int ks = 0; ks < CP / 4; ++ks) {
      const float av = dp[4 * ks];
#pragma unroll
      for (int nt = 0; nt < CT; ++nt)
        d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, As[(16 * nt + li) * LD + 4 * ks + kq], d[nt], 0, 0, 0);
    }
    float* op = dwo_part + (int64_t)b * C * C + h * c;
#pragma unroll
    for (int nt = 0; nt < CT; ++nt) {
      const int i = 16 * nt + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wv + 4 * kq + r;
        if (row < C && i < c) op[(int64_t)row * C + i] = d[nt][r];
      }
    }
    return;
  }

  // ---- dA and everything behind it
  float* Ws = sm;                      // [KR][LD]
  float* Ds = Ws + ATT_KR * LD;        // [KR][LD]
  float* colp = Ds + ATT_KR * LD;      // [16][CP]
  float* rks = colp + 16 * CP;         // [CP]
  float* red = rks + 2 * CP;           // [4]
  const float* wob = wo + h * c;
  constexpr int NLD = (ATT_KR * CP + 255) / 256;     // staged elements per thread and operand
  float wr[NLD], dr[NLD];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = t + 256 * u, rr = e / CP, j = e - rr * CP;
      const bool in = e < ATT_KR * CP && k0 + rr < C && j < c;
      wr[u] = in ? wob[(int64_t)(k0 + rr) * C + j] : 0.f;
      dr[u] = in ? dMb[(int64_t)(k0 + rr) * C + j] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = t + 256 * u, rr = e / CP, j = e - rr * CP;
      if (e < ATT_KR * CP) { Ws[rr * LD + j] = wr[u]; Ds[rr * LD + j] = dr[u]; }
    }
  };
  fetch(0);
  // A and P in the accumulator layout: rows 16 mt + 4 kq + r, column 16 nt + li
  float av[MB][CT][4], pv[MB][CT][4];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nt = 0; nt < CT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (wv + 4 * mb) + 4 * kq + r, j = 16 * nt + li;
        const bool in = i < c && j < c;
        av[mb][nt][r] = in ? Az[i * c + j] : 0.f;
        pv[mb][nt][r] = in ? P[(int64_t)z * c * c + i * c + j] : 0.f;
      }
  f32x4 acc[MB][CT];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nt = 0; nt < CT; ++nt) acc[mb][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < C; k0 += ATT_KR) {
    __syncthreads();
    stage();
    __syncthreads();
    if (k0 + ATT_KR < C) fetch(k0 + ATT_KR);
#pragma unroll
    for (int ks = 0; ks < ATT_KR / 4; ++ks) {
      float bv[CT];
#pragma unroll
      for (int nt = 0; nt < CT; ++nt) bv[nt] = Ds[(4 * ks + kq) * LD + 16 * nt + li];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int mt = wv + 4 * mb;
        if (mt < CT) {
          const float a = Ws[(4 * ks + kq) * LD + 16 * mt + li];
#pragma unroll
          for (int nt = 0; nt < CT; ++nt) acc[mb][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[nt], acc[mb][nt], 0, 0, 0);
        }
      }
    }
  }
  const float temp = temperature[h];
  const float* nz = nrm + (int64_t)z * 2 * c;
  float tsum = 0.f, colsum[CT], rq[MB][4];
#pragma unroll
  for (int nt = 0; nt < CT; ++nt) colsum[nt] = 0.f;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float dot = 0.f;
#pragma unroll
      for (int nt = 0; nt < CT; ++nt) dot += acc[mb][nt][r] * av[mb][nt][r];
      dot = row16_sum(dot);
      float rqa = 0.f;
#pragma unroll
      for (int nt = 0; nt < CT; ++nt) {
        const float ds = av[mb][nt][r] * (acc[mb][nt][r] - dot);      // (zero outside the c x c block: av is)
        const float sp = ds * pv[mb][nt][r];
        tsum += sp;
        rqa += sp * temp;
        colsum[nt] += sp * temp;
        acc[mb][nt][r] = ds;
      }
      rq[mb][r] = row16_sum(rqa);
    }
#pragma unroll
  for (int nt = 0; nt < CT; ++nt) colp[(4 * wv + kq) * CP + 16 * nt + li] = colsum[nt];
  tsum = wave_sum(tsum);
  if (lane == 0) red[wv] = tsum;
  __syncthreads();
  if (t == 0) dtemp_part[z] = (red[0] + red[1]) + (red[2] + red[3]);
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
  // vec (attn_small_plan: c % 4 == 0): 4 consecutive rows of a lane are one vector store into the transposed blocks
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int mt = wv + 4 * mb;
    if (mt >= CT) continue;
    const int i0 = 16 * mt + 4 * kq;
    float nq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) nq[r] = i0 + r < c ? nz[i0 + r] : 1.f;
#pragma unroll
    for (int nt = 0; nt < CT; ++nt) {
      const int j = 16 * nt + li;
      if (j >= c) continue;
      const float nk = nz[c + j];
      float g1[4], dq_[4], dk_[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + r;
        g1[r] = temp * acc[mb][nt][r] / (nq[r] * nk);
        // diagonal blocks: projection terms of d(x/|x|); zero when the norm was clamped
        const bool dg = i == j;
        dq_[r] = (dg && nq[r] > NORM_EPS) ? -rq[mb][r] / (nq[r] * nq[r]) : 0.f;
        dk_[r] = (dg && nk > NORM_EPS) ? -rks[j] / (nk * nk) : 0.f;
        if (i < c) {
          wq[i * 2 * c + j] = g1[r];            // dq_i += g1 * k_j
          wq[i * 2 * c + c + j] = dq_[r];
          wk[i * 2 * c + j] = dk_[r];
          if (bq) { bq[i * 2 * c + j] = (bf16)g1[r]; bq[i * 2 * c + c + j] = (bf16)dq_[r]; bk[i * 2 * c + j] = (bf16)dk_[r]; }
        }
      }
      // dk_j += g1 * q_i: the transposed block, 4 consecutive i per lane
      if (vec && i0 + 3 < c) {
        *reinterpret_cast<f32x4*>(wk + j * 2 * c + c + i0) = (f32x4){g1[0], g1[1], g1[2], g1[3]};
        if (bk) *reinterpret_cast<u32x2*>(bk + j * 2 * c + c + i0) = (u32x2){cvt_pk_bf16(g1[0], g1[1]), cvt_pk_bf16(g1[2], g1[3])};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (i0 + r < c) {
            wk[j * 2 * c + c + i0 + r] = g1[r];
            if (bk) bk[j * 2 * c + c + i0 + r] = (bf16)g1[r];
          }
      }
    }
  }
}

// per-channel sum over batch and pixels:  part[split][c] = sum x[b][c][n-range]
// The (image, vector) items of a workgroup form one index space walked with four loads in flight per thread: as a loop over the
// images with one dependent load each this kernel took an HBM round trip per image (19 us per call at bs 8 on MoCE-IR's planes).
template <typename T>
__global__ __launch_bounds__(256) void chan_sum_kernel(const T* __restrict__ x, float* __restrict__ part, int B, int C,
                                                       int64_t N, int64_t per_split, int vec) {
  __shared__ float red[4];
  const int c = blockIdx.x, sp = blockIdx.y;
  const int64_t nb = (int64_t)sp * per_split;
  int64_t ne = nb + per_split;
  if (ne > N) ne = N;
  float acc = 0.f;
  constexpr int V = 16 / (int)sizeof(T);                // elements per 16-byte load
  // (vec, decided by chan_sum_plan: whole 16-byte vectors - N, the split bounds and the base pointer allow it; a 2-byte load per
  //  lane made this kernel instruction-bound: 34 us per call on MoCE-IR's planes, 7 % of its step)
  if (vec && ne > nb) {
    const int64_t nvec = (ne - nb) / V, items = (int64_t)B * nvec;
    const T* base = x + (int64_t)c * N + nb;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i0 = threadIdx.x; i0 < items; i0 += 4 * 256) {
      float v[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + 256 * u;
        const int64_t b = i / nvec, k = i - b * nvec;
        if (i < items) Vec<T, V>::ld(base + b * C * N + k * V, v[u]);
        else {
#pragma unroll
          for (int j = 0; j < V; ++j) v[u][j] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < V; ++j) a4[u] += v[u][j];
    }
    acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  } else {
    for (int b = 0; b < B; ++b) {
      const T* row = x + ((int64_t)b * C + c) * N;
      for (int64_t n = nb + threadIdx.x; n < ne; n += 256) acc += ld1(row + n);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)sp * C + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// What one chan_sum call runs: filled by chan_sum_plan, the ONE place that decides it; launch_chan_sum launches what it says,
// chan_sum_workspace sizes from it, mi_chan_sum_plan reports it.
struct ChanSumPlan {
  int splits;        // pixel ranges (grid.y): about 512 workgroups, at least 1024 pixels each
  int64_t per;       // pixels per split, a multiple of 8 (16-byte vectors of either dtype); the last split ends at N
  int vec;           // whole 16-byte loads: every split bound is then a multiple of the vector, so N % V == 0 and a 16-byte base decide
};
static ChanSumPlan chan_sum_plan(int C, int64_t N, int dtype, bool aligned) {
  ChanSumPlan p;
  int s = 512 / (C > 0 ? C : 1);
  if (s < 1) s = 1;
  const int maxs = cdiv(N, 1024);
  if (s > maxs) s = maxs;
  p.splits = s < 1 ? 1 : s;
  p.per = (N + p.splits - 1) / p.splits;
  p.per = (p.per + 7) / 8 * 8;
  const int64_t V = 16 / (int64_t)dtype_size(dtype);
  p.vec = (N % V == 0 && aligned) ? 1 : 0;
  return p;
}
size_t chan_sum_workspace(int C, int64_t N) { return align_up((size_t)chan_sum_plan(C, N, MI_F32, true).splits * C * sizeof(float), 256); }

int launch_chan_sum(const void* x, float* out, int B, int C, int64_t N, int dtype, int accumulate, void* ws, hipStream_t st) {
  return with_dtype(dtype, "chan_sum", [&](auto tag) -> int {
    using T = decltype(tag);
    const ChanSumPlan p = chan_sum_plan(C, N, dtype, aligned16(x));
    float* part = (float*)ws;
    if (accumulate) {          // a parameter gradient accumulated in place: the split sum may wait for mi_deferred_flush (common.h)
      float* arena = deferred_take((size_t)p.splits * C, st);
      if (arena) part = arena;
    }
    ProfScope ps(st, K_CHAN_SUM, (double)B * C * N * sizeof(T), (double)B * C * N);
    hipLaunchKernelGGL((chan_sum_kernel<T>), dim3(C, p.splits), dim3(256), 0, st, (const T*)x, part, B, C, N, p.per, p.vec);
    MI_LAUNCH_CHECK();
    return launch_reduce_rows(part, out, p.splits, C, C, accumulate, 1.0f, st);
  });
}

#define ATTN_CT_SWITCH(ct, CALL)                                       \
  do {                                                                 \
    switch (ct) {                                                      \
      case 1: { constexpr int CT = 1; CALL; } break;                   \
      case 2: { constexpr int CT = 2; CALL; } break;                   \
      case 3: { constexpr int CT = 3; CALL; } break;                   \
      case 4: { constexpr int CT = 4; CALL; } break;                   \
      case 6: { constexpr int CT = 6; CALL; } break;                   \
      default: { constexpr int CT = 8; CALL; } break;                  \
    }                                                                  \
  } while (0)

size_t attn_bwd_scratch_floats(int B, int C, int heads) {
  (void)B; (void)C; (void)heads;
  return 64;            // (the one-launch backward keeps dA in registers: nothing to stage; the carve stays for the ABI)
}

// What the two launches of the c x c side run: filled by attn_small_plan, the ONE place that decides it; launch_attn_fold and
// launch_attn_bwd_small launch what it says, mi_attn_small_plan reports it.
struct AttnSmallPlan {
  int ct, promoted, cp;                     // instance CT of both kernels (1, 2, 3, 4, 6, 8); ceil(c/16) of 5 / 7 runs the next one; 16 CT
  int rpw, fold_gx, fold_gy, last_chunks;   // W_o row chunks per fold workgroup, its grid, chunks of the last row group
  size_t fold_lds, bwd_lds;                 // dynamic LDS bytes
  int fold_raise, bwd_raise;                // above 64 KiB: the kernel's limit is raised before the launch
  int bwd_gx, bwd_gy, mb;                   // backward grid; row blocks of dA a wave owns
  int tb_vec, wd_vec;                       // 4 consecutive rows of a lane are one vector store: into Mtb (C % 4 == 0), into wd / wdb (c % 4 == 0)
};
static int attn_small_plan(int B, int C, int heads, AttnSmallPlan* p) {
  MI_CHECK_ARG(B >= 1 && C >= 1 && heads >= 1, "mdta: bad shape B=%d C=%d heads=%d in the attention c x c side", B, C, heads);
  const int c = C / heads;
  MI_CHECK_ARG(c >= 1 && c <= ATTN_MAX_C && c * heads == C, "mdta: channels per head %d unsupported (1..%d)", c, ATTN_MAX_C);
  const int ct = attn_ct(c);
  p->ct = ct == 5 ? 6 : (ct == 7 ? 8 : ct);
  p->promoted = p->ct != ct;
  p->cp = 16 * p->ct;
  // row chunks per workgroup: every workgroup redoes the softmax, so deep levels (many heads, many chunks) fold several chunks
  // each; about 768 workgroups (3 per CU) are kept.  At most 8, and no more than there are: the fold's LDS holds rpw chunks.
  // (The cap at the chunk count used to come first and skip the 8: B heads > 768 with more than 8 chunks folded them all, up to
  //  48: 160 images of C = 370 in 5 heads asked for 24 chunks and 183 KiB of LDS, a launch error.)
  const int Z = B * heads, rch = attn_rchunks(C), cap = rch < 8 ? rch : 8;
  const int64_t want = ((int64_t)Z * rch) / 768;
  p->rpw = want < 1 ? 1 : (want > cap ? cap : (int)want);
  p->fold_gx = Z;
  p->fold_gy = cdiv(rch, p->rpw);
  p->last_chunks = rch - (p->fold_gy - 1) * p->rpw;
  p->fold_lds = attn_fold_lds_floats(p->ct, p->rpw) * sizeof(float);
  p->fold_raise = p->fold_lds > 64 * 1024;
  p->bwd_gx = Z;
  p->bwd_gy = 1 + cdiv(C, ATT_RW);
  p->bwd_lds = attn_bwd_lds_floats(p->ct) * sizeof(float);
  p->bwd_raise = p->bwd_lds > 64 * 1024;
  p->mb = (p->ct + 3) / 4;
  p->tb_vec = (C & 3) == 0;
  p->wd_vec = (c & 3) == 0;
  return MI_OK;
}

int launch_attn_fold(const float* graw, const float* ss, const float* temperature, const float* wo, float* P, float* A,
                     float* nrm, float* M, int B, int C, int heads, hipStream_t st, void* Mb, void* Mtb) {
  AttnSmallPlan p;
  MI_TRY(attn_small_plan(B, C, heads, &p));
  MI_CHECK_ARG(graw && ss && temperature && wo && P && A && nrm && M, "mdta: null pointer in the attention fold");
  const int c = C / heads;
  ProfScope ps(st, K_ATTN_FOLD, 4.0 * B * (3.0 * C * c + 2.0 * C * C), 2.0 * B * C * (double)c * C);
  ATTN_CT_SWITCH(p.ct, {
    if (p.fold_raise)
      MI_CHECK_HIP(hipFuncSetAttribute((const void*)attn_fold_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fold_lds));
    hipLaunchKernelGGL((attn_fold_kernel<CT>), dim3(p.fold_gx, p.fold_gy), dim3(256), p.fold_lds, st, graw, ss, temperature, wo, P, A, nrm,
                       M, (bf16*)Mb, (bf16*)Mtb, C, heads, p.rpw, p.tb_vec);
  });
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int launch_attn_bwd_small(const float* dM, const float* A, const float* P, const float* nrm, const float* temperature,
                          const float* wo, float* dwo_part, float* dtemp_part, float* wd, float* scratch,
                          int B, int C, int heads, hipStream_t st, void* wdb) {
  (void)scratch;
  AttnSmallPlan p;
  MI_TRY(attn_small_plan(B, C, heads, &p));
  MI_CHECK_ARG(dM && A && P && nrm && temperature && wo && dwo_part && dtemp_part && wd, "mdta: null pointer in the attention backward");
  const int c = C / heads;
  ProfScope ps(st, K_ATTN_BWD_SMALL, 4.0 * B * (6.0 * C * c + 3.0 * C * C), 4.0 * B * C * (double)c * C);
  ATTN_CT_SWITCH(p.ct, {
    if (p.bwd_raise)
      MI_CHECK_HIP(hipFuncSetAttribute((const void*)attn_bwd_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bwd_lds));
    hipLaunchKernelGGL((attn_bwd_kernel<CT>), dim3(p.bwd_gx, p.bwd_gy), dim3(256), p.bwd_lds, st, dM, A, P, nrm, temperature, wo,
                       dwo_part, dtemp_part, wd, (bf16*)wdb, C, heads, p.wd_vec);
  });
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // namespace mi

// The c x c side of MDTA by itself (tests, and callers that build their own attention): thin wrappers over the two launchers.
//  fwd: graw [Z,c,c] = q k^T, ss [Z,2c] = (|q_i|^2, |k_j|^2), Z = B heads -> P, A [Z,c,c], nrm [Z,2c], M [B,C,C] (fp32) and the
//       bf16 copies Mb = M, Mtb = M^T per image (either may be NULL).
//  bwd: dM [B,C,C] -> dwo_part [B,C,C] (summed over images: dW_o), dtemp_part [Z] (summed over images: d temperature),
//       wd [Z,2c,2c] = [[G1, diag D1], [diag D2, G1^T]] and its bf16 copy wdb (may be NULL).
extern "C" int mi_attn_small_fwd(const float* graw, const float* ss, const float* temperature, const float* wo, float* P, float* A,
                                 float* nrm, float* M, void* Mb, void* Mtb, int B, int C, int heads, void* stream) {
  return mi::launch_attn_fold(graw, ss, temperature, wo, P, A, nrm, M, B, C, heads, (hipStream_t)stream, Mb, Mtb);
}
extern "C" int mi_attn_small_bwd(const float* dM, const float* A, const float* P, const float* nrm, const float* temperature,
                                 const float* wo, float* dwo_part, float* dtemp_part, float* wd, void* wdb, int B, int C, int heads,
                                 void* stream) {
  return mi::launch_attn_bwd_small(dM, A, P, nrm, temperature, wo, dwo_part, dtemp_part, wd, nullptr, B, C, heads, (hipStream_t)stream,
                                   wdb);
}
// What the two launches run for B images of C channels in `heads` heads.  Host-side only: the same attn_small_plan.  out[16]:
// instance CT, promoted (ceil(c/16) of 5 or 7 runs CT 6 or 8), padded width 16 CT, W_o row chunks per fold workgroup, fold grid x,
// fold grid y, chunks in the last row group, fold LDS bytes, fold raises the 64 KiB limit, backward grid x, backward grid y,
// backward LDS bytes, backward raises the limit, row blocks of dA per wave, Mtb stored as vectors, wd / wdb stored as vectors.
extern "C" int mi_attn_small_plan(int B, int C, int heads, int64_t* out) {
  MI_CHECK_ARG(out, "attn_small_plan: null pointer");
  mi::AttnSmallPlan p;
  MI_TRY(mi::attn_small_plan(B, C, heads, &p));
  const int64_t v[16] = {p.ct, p.promoted, p.cp, p.rpw, p.fold_gx, p.fold_gy, p.last_chunks, (int64_t)p.fold_lds, p.fold_raise,
                         p.bwd_gx, p.bwd_gy, (int64_t)p.bwd_lds, p.bwd_raise, p.mb, p.tb_vec, p.wd_vec};
  memcpy(out, v, sizeof(v));
  return MI_OK;
}

// Per-channel sum over batch and pixels - the bias gradient of any conv (nn.Conv2d(bias=True): Restormer.py:82-86 with bias,
// moce_ir.py expert / decoder projections): out[c] (+)= sum_{b,n} x[b][c][n].  ws: mi_chan_sum_workspace(C, N) bytes.
extern "C" size_t mi_chan_sum_workspace(int C, int64_t N) { return (C > 0 && N > 0) ? mi::chan_sum_workspace(C, N) : 0; }
// What mi_chan_sum runs for x [B,C,N] of `dtype` whose base pointer is (aligned != 0) or is not on a 16-byte boundary.  Host-side
// only: the same chan_sum_plan.  out[4]: splits, pixels per split, vector path, workspace bytes.
extern "C" int mi_chan_sum_plan(int B, int C, int64_t N, int dtype, int aligned, int64_t* out) {
  MI_CHECK_ARG(out, "chan_sum_plan: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "chan_sum_plan: bad dtype %d", dtype);
  MI_CHECK_ARG(B >= 1 && C >= 1 && N >= 1, "chan_sum_plan: bad shape B=%d C=%d N=%lld", B, C, (long long)N);
  const mi::ChanSumPlan p = mi::chan_sum_plan(C, N, dtype, aligned != 0);
  const int64_t v[4] = {p.splits, p.per, p.vec, (int64_t)mi::chan_sum_workspace(C, N)};
  memcpy(out, v, sizeof(v));
  return MI_OK;
}
extern "C" int mi_chan_sum(const void* x, float* out, int B, int C, int64_t N, int dtype, int accumulate, void* ws, void* stream) {
  MI_CHECK_ARG(x && out && ws && B >= 1 && C >= 1 && N >= 1, "chan_sum: null pointer / bad shape");
  return mi::launch_chan_sum(x, out, B, C, N, dtype, accumulate, ws, (hipStream_t)stream);
}
