// DarkIR's dilated-gate decoder block (DBlock, DarkIR-main/archs/arch_model.py:72-139) as one C-ABI unit (mi_dblock_*), and its
// stencils on their own (mi_dilgate_*, mi_pairconv3x3_*).
//
// dilgate: the n dilated depthwise 3x3 convs of the Branch list read the same planes, so their sum is ONE sparse stencil: a shared
// centre tap (the centre weights add up, as the biases do) and 8 taps per dilation.  A workgroup stages a 32-row tile of the two
// planes of a gate pair (j, j + c) with a max(d) halo in LDS (zero outside the plane: the convs' padding, so a plane smaller
// than the halo needs no special case), forms both halves, their product g, and the tile's sum of g for the SCA pool.  Tile
// width 64 (32 when W <= 32): a wave reads 64 (2 x 32) consecutive floats of a tile row whatever the dilation - a dilation
// shifts the whole wave's read, so ds_read_b32 stays conflict-free - and the halo re-reads (1.5-2.4x the tile at d = 9) are the
// neighbour tiles' rows, in L2.  Pool partials [tile][B c] are summed over tiles by launch_reduce_rows: a fixed order, no atomics.
// Backward RECOMPUTES z from the conv input x (saved anyway, for the weight gradients): pass 1 stages x, forms z, dz = (dg + add) z~
// at the tile's own pixels, writes dz and accumulates the tap / bias gradients (per-workgroup partial rows, fixed-order sums);
// pass 2 is the same stencil with the taps mirrored over dz.  Against a stored z that costs 2c fp32 planes written and read back (dz)
// instead of 2c planes written by the forward, read by the backward and kept alive between the two.
// pairconv3x3: extra_conv (groups = c on 2c channels: a 2 x 2 channel mix per group), same tiles with a 1-pixel halo.
// The c x c folds: M[b] = diag(beta) W3 diag(s[b]) (and diag(gamma) W5) feed ONE per-image mi_pw_gemm each with the residual in
// its epilogue; their backward starts from the per-image Gram dY g^T (mi_gram, sum_batch = 0) and per-image channel sums of dY.
// With bf16 activations the 1x1 products run on split weights ([hi | lo] . [x ; x], dk_split_kernel): see there.
// The encoder block (EBlock, arch_model.py:141-204; mi_eblock_*) shares DBlock's first half: one layout, one forward and one
// backward (gh_*, "gated half") run for both, around each block's own extra_conv (EBlock's is a plain depthwise one in front of
// conv1).  Its second half is mi_fremlp_* behind norm2 and its own streaming tail out = y (1 + gamma f) (mi_fregate_*).
#include "internal.h"

namespace mi {

constexpr int DG_TH = 32, DG_MAX_D = 16, DG_MAX_N = 4, DG_MAX_SPLITS = 16, DG_NACC = 68;
constexpr int DB_MAX_C = 256;

struct DgW { const float* w[DG_MAX_N]; const float* b[DG_MAX_N]; int d[DG_MAX_N]; int n; };
struct DgPlan { int tw, th, R, lw, lh, tiles_x, tiles_y, tiles, splits; size_t lds, fwd_ws, part_floats, bwd_ws; };

static DgPlan dg_plan(int B, int c, int H, int W, int n, int R, int dtype) {
  DgPlan p;
  p.tw = W > 32 ? 64 : 32;
  p.th = DG_TH;
  p.R = R;
  p.lw = p.tw + 2 * R;
  p.lh = p.th + 2 * R;
  p.tiles_x = cdiv(W, p.tw);
  p.tiles_y = cdiv(H, p.th);
  p.tiles = p.tiles_x * p.tiles_y;
  p.splits = p.tiles < DG_MAX_SPLITS ? p.tiles : DG_MAX_SPLITS;
  p.lds = (size_t)2 * p.lw * p.lh * sizeof(float);
  p.fwd_ws = fbytes((size_t)p.tiles * B * c);
  p.part_floats = (size_t)B * p.splits * n * 2 * c * 10;     // rows [B splits] of [n][2c][9] taps, then [n][2c] biases
  p.bwd_ws = fbytes((size_t)B * 2 * c * H * W) + fbytes(p.part_floats);   // dz (fp32 in either dtype) and the partial rows
  return p;
}

static int dg_check(int B, int c, int H, int W, int n, const int* dil, int dtype, int* R) {
  MI_CHECK_ARG(B > 0 && B <= 65535 && c > 0 && c <= 65535 && H > 0 && W > 0, "dilgate: bad shape B=%d c=%d H=%d W=%d", B, c, H, W);
  MI_CHECK_ARG(n >= 1 && n <= DG_MAX_N, "dilgate: n_dil=%d not covered (1 <= n_dil <= %d)", n, DG_MAX_N);
  MI_CHECK_ARG(dil, "dilgate: null dilation list");
  int r = 0;
  for (int i = 0; i < n; ++i) {
    MI_CHECK_ARG(dil[i] >= 1 && dil[i] <= DG_MAX_D, "dilgate: dilation %d not covered (1 <= d <= %d)", dil[i], DG_MAX_D);
    r = dil[i] > r ? dil[i] : r;
  }
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "dilgate: bad dtype %d", dtype);
  MI_CHECK_ARG((int64_t)cdiv(W, 32) * cdiv(H, DG_TH) < (1ll << 31), "dilgate: plane too large");
  *R = r;
  return MI_OK;
}

// plane tile (rows ty0 - R .. ty0 + 31 + R, columns tx0 - R .. tx0 + TW - 1 + R) -> L [lh][lw]; zero outside the plane
template <typename T, int TW>
__device__ __forceinline__ void dg_load(float* L, const T* __restrict__ p, int H, int W, int ty0, int tx0, int R, int lw, int lh) {
  const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
  for (int ly = ty; ly < lh; ly += 256 / TW) {
    const int y = ty0 - R + ly;
    const bool yin = y >= 0 && y < H;
    for (int lx = tx; lx < lw; lx += TW) {
      const int x = tx0 - R + lx;
      float v = 0.f;
      if (yin && x >= 0 && x < W) v = ld1(p + (int64_t)y * W + x);
      L[ly * lw + lx] = v;
    }
  }
}

// z0[j] += sum_i sum_t w_i[ch0][t] L0[row ly + NR j, column lx, shifted by S d_i (t / 3 - 1, t % 3 - 1)], z1 likewise from L1 with
// the weights of ch1.  S = +1: the convs; -1: their transposes (the data gradient).  The centre taps are summed first.
template <int RPT, int NR, int S>
__device__ __forceinline__ void dg_conv(const float* L0, const float* L1, const DgW& a, int ch0, int ch1, int ly, int lx, int R,
                                        int lw, float (&z0)[RPT], float (&z1)[RPT]) {
  float c0 = 0.f, c1 = 0.f;
  const int base = (ly + R) * lw + lx + R;
#pragma unroll
  for (int i = 0; i < DG_MAX_N; ++i) {
    if (i < a.n) {
      const float* w0 = a.w[i] + (int64_t)ch0 * 9;
      const float* w1 = a.w[i] + (int64_t)ch1 * 9;
      const int d = S * a.d[i];
      c0 += w0[4];
      c1 += w1[4];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t == 4) continue;
        const int off = base + (t / 3 - 1) * d * lw + (t % 3 - 1) * d;
        const float u0 = w0[t], u1 = w1[t];
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
          z0[j] = fmaf(u0, L0[off + j * NR * lw], z0[j]);
          z1[j] = fmaf(u1, L1[off + j * NR * lw], z1[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    z0[j] = fmaf(c0, L0[base + j * NR * lw], z0[j]);
    z1[j] = fmaf(c1, L1[base + j * NR * lw], z1[j]);
  }
}

__device__ __forceinline__ float dg_bias_sum(const DgW& a, int ch) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < DG_MAX_N; ++i)
    if (i < a.n && a.b[i]) s += a.b[i][ch];
  return s;
}

// grid (tiles, c, B).  GATE: x [B][2c] -> g [B][c] and the tile's sum of g -> pool_part[tile][b c + j].
// !GATE: the transposed stencil per plane: x = dz [B][2c] (TI = float) -> out = dx [B][2c] (no bias).
template <typename TI, typename T, int TW, bool GATE>
__global__ __launch_bounds__(256) void dilgate_kernel(const TI* __restrict__ x, DgW a, T* __restrict__ out, float* __restrict__ pool_part,
                                                      int c, int H, int W, int tiles_x, int R) {
  constexpr int NR = 256 / TW, RPT = DG_TH / NR;
  extern __shared__ float dg_lds[];
  __shared__ float red[4];
  const int lw = TW + 2 * R, lh = DG_TH + 2 * R, lt = lw * lh;
  const int j = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * DG_TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int64_t N = (int64_t)H * W, p0 = ((int64_t)b * 2 * c + j) * N, p1 = p0 + (int64_t)c * N;
  float* L0 = dg_lds;
  float* L1 = dg_lds + lt;
  dg_load<TI, TW>(L0, x + p0, H, W, ty0, tx0, R, lw, lh);
  dg_load<TI, TW>(L1, x + p1, H, W, ty0, tx0, R, lw, lh);
  __syncthreads();
  const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
  float z0[RPT], z1[RPT];
  const float b0 = GATE ? dg_bias_sum(a, j) : 0.f, b1 = GATE ? dg_bias_sum(a, j + c) : 0.f;
#pragma unroll
  for (int r = 0; r < RPT; ++r) { z0[r] = b0; z1[r] = b1; }
  dg_conv<RPT, NR, GATE ? 1 : -1>(L0, L1, a, j, j + c, ty, tx, R, lw, z0, z1);
  const int xx = tx0 + tx;
  float ps = 0.f;
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int y = ty0 + ty + r * NR;
    if (xx < W && y < H) {
      const int64_t o = (int64_t)y * W + xx;
      if (GATE) {
        const float gv = z0[r] * z1[r];
        st1(out + ((int64_t)b * c + j) * N + o, gv);
        ps += gv;
      } else {
        st1(out + p0 + o, z0[r]);
        st1(out + p1 + o, z1[r]);
      }
    }
  }
  if (GATE) {
    const float s = wave_sum(ps);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
      pool_part[(int64_t)blockIdx.x * gridDim.z * c + (int64_t)b * c + j] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// Sums NV per-thread values over the workgroup (wave DPP sums, then the 4 waves in order); thread n < NV gets total n.
template <int NV>
__device__ __forceinline__ float dk_block_sum(const float (&v)[NV], float* red) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    const float s = wave_sum(v[n]);
    if (lane == 0) red[wv * NV + n] = s;
  }
  __syncthreads();
  const int n = threadIdx.x;
  return n < NV ? (red[n] + red[NV + n]) + (red[2 * NV + n] + red[3 * NV + n]) : 0.f;
}

// Backward pass 1, grid (splits, c, B): over the tiles split, split + splits, ...: z from x, dz = (dg + add) (the other half of z)
// -> dz [B][2c] (fp32 whatever the activation dtype: scratch between the two passes, not rounded a second time); the tap and bias gradients of every branch -> partial row (b splits + split).  A thread's accumulators: half e
// (channel j + e c) at acc[34 e ..]: 8 off-centre taps of branch i at [8 i ..], the centre tap (shared by the branches) at [32],
// the bias (shared too) at [33].  Row layout: [n][2c][9] taps, then [n][2c] biases (part_ld floats).
template <typename T, int TW>
__global__ __launch_bounds__(256) void dilgate_bwd_dz_kernel(const T* __restrict__ dg, const float* __restrict__ dg_add,
                                                             const T* __restrict__ x, DgW a, float* __restrict__ dz, float* __restrict__ part,
                                                             int64_t part_ld, int c, int H, int W, int tiles_x, int ntiles, int R) {
  constexpr int NR = 256 / TW, RPT = DG_TH / NR;
  extern __shared__ float dg_lds[];
  __shared__ float red[4 * DG_NACC];
  const int lw = TW + 2 * R, lh = DG_TH + 2 * R, lt = lw * lh;
  const int split = blockIdx.x, splits = gridDim.x, j = blockIdx.y, b = blockIdx.z;
  const int64_t N = (int64_t)H * W, p0 = ((int64_t)b * 2 * c + j) * N, p1 = p0 + (int64_t)c * N, pg = ((int64_t)b * c + j) * N;
  float* L0 = dg_lds;
  float* L1 = dg_lds + lt;
  const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
  const float b0 = dg_bias_sum(a, j), b1 = dg_bias_sum(a, j + c);
  const float add = dg_add ? dg_add[(int64_t)b * c + j] : 0.f;
  float acc[DG_NACC];
#pragma unroll
  for (int k = 0; k < DG_NACC; ++k) acc[k] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * DG_TH, tx0 = (tile % tiles_x) * TW;
    __syncthreads();
    dg_load<T, TW>(L0, x + p0, H, W, ty0, tx0, R, lw, lh);
    dg_load<T, TW>(L1, x + p1, H, W, ty0, tx0, R, lw, lh);
    __syncthreads();
    const int xx = tx0 + tx;
    // one tile row of the thread at a time: the 68 accumulators stay in registers beside one row's z, dz and tap loads
#pragma unroll 1
    for (int r = 0; r < RPT; ++r) {
      const int ly = ty + r * NR, y = ty0 + ly;
      float z0[1] = {b0}, z1[1] = {b1};
      dg_conv<1, NR, 1>(L0, L1, a, j, j + c, ly, tx, R, lw, z0, z1);
      float d0 = 0.f, d1 = 0.f;
      if (xx < W && y < H) {
        const int64_t o = (int64_t)y * W + xx;
        const float gv = ld1(dg + pg + o) + add;
        d0 = gv * z1[0];
        d1 = gv * z0[0];
        dz[p0 + o] = d0;
        dz[p1 + o] = d1;
      }
      const int base = (ly + R) * lw + tx + R;
#pragma unroll
      for (int i = 0; i < DG_MAX_N; ++i) {
        if (i < a.n) {
          const int d = a.d[i];
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            if (t == 4) continue;
            const int tt = t < 4 ? t : t - 1;
            const int off = base + (t / 3 - 1) * d * lw + (t % 3 - 1) * d;
            acc[8 * i + tt] = fmaf(d0, L0[off], acc[8 * i + tt]);
            acc[34 + 8 * i + tt] = fmaf(d1, L1[off], acc[34 + 8 * i + tt]);
          }
        }
      }
      acc[32] = fmaf(d0, L0[base], acc[32]);
      acc[66] = fmaf(d1, L1[base], acc[66]);
      acc[33] += d0;
      acc[67] += d1;
    }
  }
  const float tot = dk_block_sum<DG_NACC>(acc, red);
  const int n = threadIdx.x;
  if (n >= DG_NACC) return;
  const int e = n / 34, r = n - 34 * e, C2 = 2 * c, ch = j + e * c;
  float* row = part + ((int64_t)b * splits + split) * part_ld;
  if (r < 32) {
    const int i = r >> 3, tt = r & 7, t = tt < 4 ? tt : tt + 1;
    if (i < a.n) row[((int64_t)i * C2 + ch) * 9 + t] = tot;
  } else if (r == 32) {
    for (int i = 0; i < a.n; ++i) row[((int64_t)i * C2 + ch) * 9 + 4] = tot;
  } else {
    for (int i = 0; i < a.n; ++i) row[(int64_t)a.n * C2 * 9 + (int64_t)i * C2 + ch] = tot;
  }
}

// ------------------------------------------------------------------ pair-grouped 3x3 (extra_conv)
constexpr int PC_R = 1;
// grid (tiles, c, B): group g = blockIdx.y, planes 2g, 2g + 1.  S = +1: out[2g + q] = bias + sum_r w[2g + q][r] * in[2g + r];
// S = -1: the data gradient out[2g + q] = sum_r w[2g + r][q]^T * in[2g + r] (taps mirrored, channel roles swapped, no bias).
template <typename T, int TW, int S>
__global__ __launch_bounds__(256) void pairconv_kernel(const T* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                       T* __restrict__ out, int c, int H, int W, int tiles_x) {
  constexpr int NR = 256 / TW, RPT = DG_TH / NR, LW = TW + 2 * PC_R, LH = DG_TH + 2 * PC_R, LT = LW * LH;
  __shared__ float L[2 * LT];
  const int g = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * DG_TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int64_t N = (int64_t)H * W, p0 = ((int64_t)b * 2 * c + 2 * g) * N;
  dg_load<T, TW>(L, in + p0, H, W, ty0, tx0, PC_R, LW, LH);
  dg_load<T, TW>(L + LT, in + p0 + N, H, W, ty0, tx0, PC_R, LW, LH);
  __syncthreads();
  const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW, xx = tx0 + tx;
  const float* wg = w + (int64_t)g * 36;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float z[RPT];
    const float bq = (S > 0 && bias) ? bias[2 * g + q] : 0.f;
#pragma unroll
    for (int r = 0; r < RPT; ++r) z[r] = bq;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float u = S > 0 ? wg[q * 18 + e * 9 + t] : wg[e * 18 + q * 9 + t];
        const int off = (ty + PC_R + S * (t / 3 - 1)) * LW + tx + PC_R + S * (t % 3 - 1);
#pragma unroll
        for (int r = 0; r < RPT; ++r) z[r] = fmaf(u, L[e * LT + off + r * NR * LW], z[r]);
      }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int y = ty0 + ty + r * NR;
      if (xx < W && y < H) st1(out + p0 + q * N + (int64_t)y * W + xx, z[r]);
    }
  }
}

// grid (splits, c, B): dw[2g + q][e][t] = sum_p dy[2g + q][p] x[2g + e][p + off(t)], db[2g + q] = sum_p dy[2g + q][p] over the
// tiles split, split + splits, ...; partial row (b splits + split) of [2c][18] weights, then [2c] biases.
template <typename T, int TW>
__global__ __launch_bounds__(256) void pairconv_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
                                                             int c, int H, int W, int tiles_x, int ntiles) {
  constexpr int NR = 256 / TW, RPT = DG_TH / NR, LW = TW + 2 * PC_R, LH = DG_TH + 2 * PC_R, LT = LW * LH;
  __shared__ float L[2 * LT];
  __shared__ float red[4 * 38];
  const int split = blockIdx.x, splits = gridDim.x, g = blockIdx.y, b = blockIdx.z;
  const int64_t N = (int64_t)H * W, p0 = ((int64_t)b * 2 * c + 2 * g) * N;
  const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
  float acc[38];
#pragma unroll
  for (int k = 0; k < 38; ++k) acc[k] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * DG_TH, tx0 = (tile % tiles_x) * TW;
    __syncthreads();
    dg_load<T, TW>(L, x + p0, H, W, ty0, tx0, PC_R, LW, LH);
    dg_load<T, TW>(L + LT, x + p0 + N, H, W, ty0, tx0, PC_R, LW, LH);
    __syncthreads();
    const int xx = tx0 + tx;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int y = ty0 + ty + r * NR;
      if (xx < W && y < H) {
        const int64_t o = (int64_t)y * W + xx;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float d = ld1(dy + p0 + q * N + o);
          acc[36 + q] += d;
#pragma unroll
          for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int t = 0; t < 9; ++t)
              acc[q * 18 + e * 9 + t] = fmaf(d, L[e * LT + (ty + r * NR + PC_R + t / 3 - 1) * LW + tx + PC_R + t % 3 - 1], acc[q * 18 + e * 9 + t]);
        }
      }
    }
  }
  const float tot = dk_block_sum<38>(acc, red);
  const int n = threadIdx.x;
  float* row = part + ((int64_t)b * splits + split) * (int64_t)c * 38;
  if (n < 36) row[(int64_t)g * 36 + n] = tot;
  else if (n < 38) row[(int64_t)c * 36 + 2 * g + n - 36] = tot;
}

// ------------------------------------------------------------------ the c x c folds
// grid (B), dynamic LDS 2c floats.  With the SCA (pool != NULL): s[b] = wsca . (pool[b] inv_n) + bsca -> s_out [B][c]; without: s = 1.
// M[b][o][k] = scale[o] w[o][k] s[b][k] (fp32); bias_out[o] = scale[o] bias[o].  Ms / Mts (bf16 activations, else NULL): M and its
// transpose as SPLIT images [c][2c] = [hi | lo], hi = M rounded to bf16, lo = M - hi (dk_split_kernel).
__global__ __launch_bounds__(256) void dk_fold_kernel(const float* __restrict__ pool, const float* __restrict__ wsca,
                                                      const float* __restrict__ bsca, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ scale,
                                                      float* __restrict__ s_out, float* __restrict__ M, float* __restrict__ Ms,
                                                      float* __restrict__ Mts, float* __restrict__ bias_out, int c, float inv_n) {
  extern __shared__ float dk_sh[];
  float* pm = dk_sh;
  float* s = dk_sh + c;
  const int b = blockIdx.x;
  if (pool) {
    for (int k = threadIdx.x; k < c; k += 256) pm[k] = pool[(int64_t)b * c + k] * inv_n;
    __syncthreads();
    for (int o = threadIdx.x; o < c; o += 256) {
      float v = bsca[o];
      for (int k = 0; k < c; ++k) v = fmaf(wsca[(int64_t)o * c + k], pm[k], v);
      s[o] = v;
      s_out[(int64_t)b * c + o] = v;
    }
  } else {
    for (int k = threadIdx.x; k < c; k += 256) s[k] = 1.f;
  }
  __syncthreads();
  const int64_t cc = (int64_t)c * c;
  for (int e = threadIdx.x; e < c * c; e += 256) {
    const int o = e / c, k = e - o * c;
    const float v = scale[o] * w[e] * s[k];
    M[b * cc + e] = v;
    if (Ms) {
      const float hi = (float)(bf16)v, lo = v - hi;
      float* r = Ms + 2 * b * cc + (int64_t)o * 2 * c + k;
      float* t = Mts + 2 * b * cc + (int64_t)k * 2 * c + o;
      r[0] = hi; r[c] = lo;
      t[0] = hi; t[c] = lo;
    }
  }
  if (b == 0)
    for (int o = threadIdx.x; o < c; o += 256) bias_out[o] = scale[o] * bias[o];
}

// The bf16 MFMA GEMMs round their weights to bf16: an error common to a whole channel, which the pixel sums of the bias gradients
// keep whole (measured: it alone put conv1.bias' gradient at 4.6x the error of bf16 storage).  The block therefore feeds them SPLIT
// weights: y = [hi | lo] . [x ; x] through mi_pw_gemm's two K panels, hi = w rounded to bf16, lo = w - hi (rounded again by the
// packer: 16 mantissa bits in all), twice the MFMA work of GEMMs that are bound by their activation traffic.
// w [M][K] -> out [M][2K] = [hi | lo];  transpose: out [K][2M], out[k][m] = hi(w[m][k]), out[k][M + m] = lo(w[m][k])
__global__ __launch_bounds__(256) void dk_split_kernel(const float* __restrict__ w, float* __restrict__ out, int M, int K, int transpose) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < M * K; e += gridDim.x * 256) {
    const int m = e / K, k = e - m * K;
    const float v = w[e], hi = (float)(bf16)v, lo = v - hi;
    float* o = transpose ? out + (int64_t)k * 2 * M + m : out + (int64_t)m * 2 * K + k;
    o[0] = hi;
    o[transpose ? M : K] = lo;
  }
}

// grid (B), dynamic LDS c floats: ds[b][k] = sum_o scale[o] w[o][k] G[b][o][k];  dg_add[b][m] = inv_n sum_k wsca[k][m] ds[b][k]
__global__ __launch_bounds__(256) void dk_sca_ds_kernel(const float* __restrict__ G, const float* __restrict__ w, const float* __restrict__ scale,
                                                        const float* __restrict__ wsca, float* __restrict__ ds, float* __restrict__ dg_add,
                                                        int c, float inv_n) {
  extern __shared__ float dk_sh[];
  const int b = blockIdx.x;
  const float* Gb = G + (int64_t)b * c * c;
  for (int k = threadIdx.x; k < c; k += 256) {
    float v = 0.f;
    for (int o = 0; o < c; ++o) v = fmaf(scale[o] * w[(int64_t)o * c + k], Gb[(int64_t)o * c + k], v);
    ds[(int64_t)b * c + k] = v;
    dk_sh[k] = v;
  }
  __syncthreads();
  for (int m = threadIdx.x; m < c; m += 256) {
    float v = 0.f;
    for (int k = 0; k < c; ++k) v = fmaf(wsca[(int64_t)k * c + m], dk_sh[k], v);
    dg_add[(int64_t)b * c + m] = v * inv_n;
  }
}

// grid (c), row o.  G [nb][c][c] (nb = B per-image Grams dY g^T, or 1: already summed), s [nb][c] or NULL (= 1), S [nb][c] the
// channel sums of dY:  dw[o][k] (+)= scale[o] sum_b s[b][k] G[b][o][k];  dbias[o] (+)= scale[o] sum_b S[b][o];
// dscale[o] (+)= sum_b (sum_k w[o][k] s[b][k] G[b][o][k] + bias[o] S[b][o])
__global__ __launch_bounds__(256) void dk_fold_bwd_kernel(const float* __restrict__ G, const float* __restrict__ s, const float* __restrict__ S,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ scale, float* __restrict__ dw, float* __restrict__ dbias,
                                                          float* __restrict__ dscale, int nb, int c, int acc) {
  __shared__ float red[4];
  const int o = blockIdx.x;
  const float sc = scale[o];
  float q = 0.f;
  for (int k = threadIdx.x; k < c; k += 256) {
    float h = 0.f;
    for (int b = 0; b < nb; ++b) h = fmaf(s ? s[(int64_t)b * c + k] : 1.f, G[((int64_t)b * c + o) * c + k], h);
    const int64_t e = (int64_t)o * c + k;
    q = fmaf(w[e], h, q);
    dw[e] = acc ? dw[e] + sc * h : sc * h;
  }
  const float t = wave_sum(q);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float Ss = 0.f;
    for (int b = 0; b < nb; ++b) Ss += S[(int64_t)b * c + o];
    const float dsc = ((red[0] + red[1]) + (red[2] + red[3])) + bias[o] * Ss, db = sc * Ss;
    dscale[o] = acc ? dscale[o] + dsc : dsc;
    dbias[o] = acc ? dbias[o] + db : db;
  }
}

// grid (c), row k: dwsca[k][m] (+)= sum_b ds[b][k] pool[b][m] inv_n;  dbsca[k] (+)= sum_b ds[b][k]
__global__ __launch_bounds__(256) void dk_sca_w_kernel(const float* __restrict__ ds, const float* __restrict__ pool, float* __restrict__ dwsca,
                                                       float* __restrict__ dbsca, int B, int c, float inv_n, int acc) {
  const int k = blockIdx.x;
  for (int m = threadIdx.x; m < c; m += 256) {
    float v = 0.f;
    for (int b = 0; b < B; ++b) v = fmaf(ds[(int64_t)b * c + k], pool[(int64_t)b * c + m] * inv_n, v);
    const int64_t e = (int64_t)k * c + m;
    dwsca[e] = acc ? dwsca[e] + v : v;
  }
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += ds[(int64_t)b * c + k];
    dbsca[k] = acc ? dbsca[k] + v : v;
  }
}

// ------------------------------------------------------------------ launchers
static DgW dg_args(const mi_dilgate_params* p, int n, const int* dil) {
  DgW a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  for (int i = 0; i < n; ++i) { a.w[i] = p->w[i]; a.b[i] = p->b[i]; a.d[i] = dil[i]; }
  return a;
}

template <typename TI, typename T, int TW, bool GATE>
static int dg_launch(const DgPlan& pl, const void* x, const DgW& a, void* out, float* part, int B, int c, int H, int W, hipStream_t st) {
  return launch_dyn_lds(dilgate_kernel<TI, T, TW, GATE>, dim3(pl.tiles, c, B), dim3(256), pl.lds, st, (const TI*)x, a, (T*)out, part, c, H, W,
                        pl.tiles_x, pl.R);
}

static int launch_dilgate_fwd(const void* x, const mi_dilgate_params* p, void* g, float* pool, int B, int c, int H, int W, int n,
                              const int* dil, int dtype, void* ws, hipStream_t st) {
  int R = 0;
  MI_TRY(dg_check(B, c, H, W, n, dil, dtype, &R));
  MI_CHECK_ARG(x && p && g && pool && ws, "dilgate_fwd: null pointer");
  for (int i = 0; i < n; ++i) MI_CHECK_ARG(p->w[i], "dilgate_fwd: null weight of branch %d", i);
  const DgPlan pl = dg_plan(B, c, H, W, n, R, dtype);
  const DgW a = dg_args(p, n, dil);
  float* part = (float*)ws;
  MI_TRY(with_dtype(dtype, "dilgate_fwd", [&](auto tag) -> int {
    using T = decltype(tag);
    const double nn = (double)B * c * H * W;
    ProfScope ps(st, K_DK_GATE_FWD, 3.0 * nn * sizeof(T), 2.0 * 2 * (8 * n + 1) * nn);
    return pl.tw == 64 ? dg_launch<T, T, 64, true>(pl, x, a, g, part, B, c, H, W, st) : dg_launch<T, T, 32, true>(pl, x, a, g, part, B, c, H, W, st);
  }));
  return launch_reduce_rows(part, pool, pl.tiles, (int64_t)B * c, (int64_t)B * c, 0, 1.0f, st);
}

static int launch_dilgate_bwd(const void* dg, const float* dg_add, const void* x, const mi_dilgate_params* p, void* dx,
                              const mi_dilgate_grads* gr, int B, int c, int H, int W, int n, const int* dil, int dtype, void* ws,
                              hipStream_t st) {
  int R = 0;
  MI_TRY(dg_check(B, c, H, W, n, dil, dtype, &R));
  MI_CHECK_ARG(dg && x && p && dx && gr && ws, "dilgate_bwd: null pointer");
  for (int i = 0; i < n; ++i) MI_CHECK_ARG(p->w[i] && gr->w[i], "dilgate_bwd: null weight or gradient of branch %d", i);
  const DgPlan pl = dg_plan(B, c, H, W, n, R, dtype);
  const DgW a = dg_args(p, n, dil);
  Carver cv(ws);
  float* dz = cv.take<float>(fbytes((size_t)B * 2 * c * H * W));
  float* part = cv.take<float>(fbytes(pl.part_floats));
  const int64_t ld = (int64_t)n * 2 * c * 10, rows = (int64_t)B * pl.splits;
  MI_TRY(with_dtype(dtype, "dilgate_bwd", [&](auto tag) -> int {
    using T = decltype(tag);
    const double nn = (double)B * c * H * W;
    {
      ProfScope ps(st, K_DK_GATE_BWD_DZ, 3.0 * nn * sizeof(T) + 8.0 * nn, 2.0 * 4 * (8 * n + 1) * nn);
      if (pl.tw == 64)
        MI_TRY(launch_dyn_lds(dilgate_bwd_dz_kernel<T, 64>, dim3(pl.splits, c, B), dim3(256), pl.lds, st, (const T*)dg, dg_add, (const T*)x,
                              a, dz, part, ld, c, H, W, pl.tiles_x, pl.tiles, pl.R));
      else
        MI_TRY(launch_dyn_lds(dilgate_bwd_dz_kernel<T, 32>, dim3(pl.splits, c, B), dim3(256), pl.lds, st, (const T*)dg, dg_add, (const T*)x,
                              a, dz, part, ld, c, H, W, pl.tiles_x, pl.tiles, pl.R));
    }
    ProfScope ps(st, K_DK_GATE_BWD_DX, 2.0 * nn * sizeof(T) + 8.0 * nn, 2.0 * 2 * (8 * n + 1) * nn);
    return pl.tw == 64 ? dg_launch<float, T, 64, false>(pl, dz, a, dx, nullptr, B, c, H, W, st)
                       : dg_launch<float, T, 32, false>(pl, dz, a, dx, nullptr, B, c, H, W, st);
  }));
  for (int i = 0; i < n; ++i) {
    MI_TRY(launch_reduce_rows(part + (int64_t)i * 2 * c * 9, gr->w[i], rows, (int64_t)2 * c * 9, ld, gr->accumulate, 1.0f, st));
    if (gr->b[i]) MI_TRY(launch_reduce_rows(part + (int64_t)n * 2 * c * 9 + (int64_t)i * 2 * c, gr->b[i], rows, 2 * c, ld, gr->accumulate, 1.0f, st));
  }
  return MI_OK;
}

static int pc_check(int B, int c, int H, int W, int dtype) {
  MI_CHECK_ARG(B > 0 && B <= 65535 && c > 0 && c <= 65535 && H > 0 && W > 0, "pairconv3x3: bad shape B=%d c=%d H=%d W=%d", B, c, H, W);
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "pairconv3x3: bad dtype %d", dtype);
  MI_CHECK_ARG((int64_t)cdiv(W, 32) * cdiv(H, DG_TH) < (1ll << 31), "pairconv3x3: plane too large");
  return MI_OK;
}
static size_t pc_part_floats(int B, int c, int H, int W) { return (size_t)B * dg_plan(B, c, H, W, 1, 1, MI_F32).splits * c * 38; }

// S = +1: y = extra_conv(x); -1: dx from dy
template <int S>
static int launch_pairconv(const void* in, const float* w, const float* bias, void* out, int B, int c, int H, int W, int dtype, hipStream_t st) {
  MI_TRY(pc_check(B, c, H, W, dtype));
  MI_CHECK_ARG(in && w && out, "pairconv3x3: null pointer");
  const DgPlan pl = dg_plan(B, c, H, W, 1, 1, dtype);
  const double nn = (double)B * 2 * c * H * W;
  ProfScope ps(st, K_DK_PAIR, 2.0 * nn * dtype_size(dtype), 2.0 * 18 * nn);
  return with_dtype(dtype, "pairconv3x3", [&](auto tag) {
    using T = decltype(tag);
    if (pl.tw == 64)
      hipLaunchKernelGGL((pairconv_kernel<T, 64, S>), dim3(pl.tiles, c, B), dim3(256), 0, st, (const T*)in, w, bias, (T*)out, c, H, W, pl.tiles_x);
    else
      hipLaunchKernelGGL((pairconv_kernel<T, 32, S>), dim3(pl.tiles, c, B), dim3(256), 0, st, (const T*)in, w, bias, (T*)out, c, H, W, pl.tiles_x);
  });
}

static int launch_pairconv_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, int B, int c, int H, int W,
                               int accumulate, int dtype, void* ws, hipStream_t st) {
  MI_TRY(pc_check(B, c, H, W, dtype));
  MI_CHECK_ARG(dy && x && w && dx && dw && ws, "pairconv3x3_bwd: null pointer");
  MI_TRY(launch_pairconv<-1>(dy, w, nullptr, dx, B, c, H, W, dtype, st));
  const DgPlan pl = dg_plan(B, c, H, W, 1, 1, dtype);
  float* part = (float*)ws;
  {
    const double nn = (double)B * 2 * c * H * W;
    ProfScope ps(st, K_DK_PAIR_WGRAD, 2.0 * nn * dtype_size(dtype), 2.0 * 19 * nn);
    MI_TRY(with_dtype(dtype, "pairconv3x3_bwd", [&](auto tag) {
      using T = decltype(tag);
      if (pl.tw == 64)
        hipLaunchKernelGGL((pairconv_wgrad_kernel<T, 64>), dim3(pl.splits, c, B), dim3(256), 0, st, (const T*)dy, (const T*)x, part, c, H, W, pl.tiles_x, pl.tiles);
      else
        hipLaunchKernelGGL((pairconv_wgrad_kernel<T, 32>), dim3(pl.splits, c, B), dim3(256), 0, st, (const T*)dy, (const T*)x, part, c, H, W, pl.tiles_x, pl.tiles);
    }));
  }
  const int64_t rows = (int64_t)B * pl.splits, ld = (int64_t)c * 38;
  MI_TRY(launch_reduce_rows(part, dw, rows, (int64_t)c * 36, ld, accumulate, 1.0f, st));
  if (db) MI_TRY(launch_reduce_rows(part + (int64_t)c * 36, db, rows, 2 * c, ld, accumulate, 1.0f, st));
  return MI_OK;
}

// ------------------------------------------------------------------ the gated half: one description for both blocks
// LayerNorm2d -> conv1 -> dilated gate -> SCA fold -> per-image conv3 with beta and the residual is the first half of DBlock and of
// EBlock alike, and so is its backward; only extra_conv differs (DBlock: pair-grouped, behind conv1; EBlock: plain depthwise, in
// front of it).  What the chain stores and what it needs as scratch is laid out once, here; a block adds its own sections.
// (S, P and G below: either block's mi_*_shape, mi_*_params and mi_*_grads, which name the chain's fields alike.)

// cin: conv1's input, x0 or an extra_conv in front of conv1 applied to it; gin: the gate's input, x1 or an extra_conv behind conv1
// applied to it.  M3s / M3ts: split images (bf16 activations).  A block has at most one extra_conv: cin or gin is a plane of its own.
struct GhSaved {
  void* x0; void* cin; void* x1; void* gin; void* g; void* y;
  float* mean1; float* rstd1; float* pool; float* s; float* M3; float* b3f; float* M3s; float* M3ts;
  size_t sec[8];     // bytes, as carved, of x0, cin, x1, gin, g, y (0 where a plane is shared), the statistics, the small tensors
};
template <typename S>
static GhSaved gh_saved_carve(Carver& cv, const S* s, bool extra_front, bool extra_behind) {
  const size_t B = s->B, C = s->C, N = (size_t)s->H * s->W, cc = B * C * C;
  const int dt = s->dtype;
  GhSaved r;
  size_t o = cv.off;
  auto close = [&](int i) { r.sec[i] = cv.off - o; o = cv.off; };
  r.x0 = cv.take(tbytes(B * C * N, dt)); close(0);
  r.cin = extra_front ? cv.take(tbytes(B * C * N, dt)) : r.x0; close(1);
  r.x1 = cv.take(tbytes(B * 2 * C * N, dt)); close(2);
  r.gin = extra_behind ? cv.take(tbytes(B * 2 * C * N, dt)) : r.x1; close(3);
  r.g = cv.take(tbytes(B * C * N, dt)); close(4);
  r.y = cv.take(tbytes(B * C * N, dt)); close(5);
  r.mean1 = cv.take<float>(fbytes(B * N));
  r.rstd1 = cv.take<float>(fbytes(B * N)); close(6);
  r.pool = cv.take<float>(fbytes(B * C));
  r.s = cv.take<float>(fbytes(B * C));
  r.M3 = cv.take<float>(fbytes(cc));
  r.b3f = cv.take<float>(fbytes(C));
  r.M3s = cv.take<float>(fbytes(2 * cc));
  r.M3ts = cv.take<float>(fbytes(2 * cc)); close(7);
  return r;
}

// y[B][M] = W x (+ bias) (+ res).  split: w is a split image [M][2K] and x enters as both K panels; per_img: one matrix per image
static mi_pw_desc db_gemm(const void* x, int K, const float* w, bool split, bool per_img, const float* bias, const void* res, void* y, int M,
                          int B, int64_t N, int dt) {
  mi_pw_desc d = conv1x1(x, K, w, false, split ? 2 * K : K, bias, res, y, M, B, N, dt);
  if (split) { d.x2 = x; d.x2_bs = d.x1_bs; d.k2 = K; }
  if (per_img) d.w_bs = (int64_t)M * (split ? 2 * K : K);
  return d;
}
// the same for W^T dy with w [M][K] given as it is (fp32 activations: no split)
static mi_pw_desc db_gemm_t(const void* dy, int M, const float* w, bool per_img, void* dx, int K, int B, int64_t N, int dt) {
  mi_pw_desc d = conv1x1(dy, M, w, true, K, nullptr, nullptr, dx, K, B, N, dt);
  if (per_img) d.w_bs = (int64_t)M * K;
  return d;
}
static size_t db_probe(int K, int M, bool split, bool per_img, bool t, int B, int64_t N, int dt) {
  const mi_pw_desc d = t ? db_gemm_t(PROBE_PTR, K, (const float*)PROBE_PTR, per_img, PROBE_PTR, M, B, N, dt)
                         : db_gemm(PROBE_PTR, K, (const float*)PROBE_PTR, split, per_img, nullptr, nullptr, PROBE_PTR, M, B, N, dt);
  return pw_ws_bytes(d);
}

// The scratch of the chain and of the 1x1 products and Grams of a block's second half, which are of the same shapes.  t1..t3: the
// backward's three [B][2c] planes (gh_ws_tail).
struct GhWs {
  void* pw_ws; void* gram_ws; void* cs_ws; void* ln_ws; void* dg_fwd_ws; void* dg_bwd_ws;
  float* G; float* S; float* ds; float* dg_add; float* wsplit;
  void* t1; void* t2; void* t3;
};
// own_gram: the workspace of a Gram that only the block's second half runs (0: none)
template <typename S>
static GhWs gh_ws_carve(Carver& cv, const S* s, int R, size_t own_gram) {
  const int B = s->B, C = s->C, dt = s->dtype;
  const int64_t N = (int64_t)s->H * s->W;
  GhWs w;
  const bool sp = dt == MI_BF16;
  // c -> 2c, its transpose 2c -> c, the per-image c -> c and its transpose (bf16: all four as split products, none transposed)
  w.pw_ws = cv.take(max_of({db_probe(C, 2 * C, sp, false, false, B, N, dt), db_probe(C, C, sp, true, false, B, N, dt),
                            sp ? db_probe(2 * C, C, true, false, false, B, N, dt) : db_probe(2 * C, C, false, false, true, B, N, dt),
                            sp ? (size_t)0 : db_probe(C, C, false, true, true, B, N, dt)}));
  w.wsplit = cv.take<float>(fbytes((size_t)4 * C * C));
  w.gram_ws = cv.take(max_of({gram_ws_bytes(probe_wgrad(C, C, B, N, dt, 0)), gram_ws_bytes(probe_wgrad(2 * C, C, B, N, dt, 1)), own_gram}));
  w.cs_ws = cv.take(chan_sum_workspace(B * C > 2 * C ? B * C : 2 * C, N));
  w.ln_ws = cv.take(mi_ln_bwd_workspace(B, C, N));
  const DgPlan pl = dg_plan(B, C, s->H, s->W, s->n_dil, R, dt);
  w.dg_fwd_ws = cv.take(pl.fwd_ws);
  w.dg_bwd_ws = cv.take(pl.bwd_ws);
  w.G = cv.take<float>(fbytes((size_t)B * C * C));
  w.S = cv.take<float>(fbytes((size_t)B * C));
  w.ds = cv.take<float>(fbytes((size_t)B * C));
  w.dg_add = cv.take<float>(fbytes((size_t)B * C));
  return w;
}
static void* ws_at(void* base, size_t off) { return base ? (char*)base + off : nullptr; }
// Behind every other section and overlaid on one another: the inference copy of the saved planes (inf_bytes at `over`; a forward
// without a blob keeps nothing) and the backward's t1..t3.  -> the bytes of the overlay
template <typename S>
static size_t gh_ws_tail(GhWs& w, void* over, size_t inf_bytes, const S* s) {
  Carver big(over);
  const size_t plane2 = tbytes((size_t)s->B * 2 * s->C * s->H * s->W, s->dtype);
  w.t1 = big.take(plane2);
  w.t2 = big.take(plane2);
  w.t3 = big.take(plane2);
  return max_of({inf_bytes, big.off});
}

// The null checks of a block's parameters (what = "parameter") or gradient buffers ("gradient buffer").  own: the fields of the
// block's second half are all set.
template <typename P>
static int gh_check_par(const char* who, const char* what, const P* p, bool own, int extra, int n_dil) {
  MI_CHECK_ARG(p->norm1_w && p->norm1_b && p->conv1_w && p->conv1_b && p->sca_w && p->sca_b && p->conv3_w && p->conv3_b && p->beta && own,
               "%s: null %s", who, what);
  MI_CHECK_ARG(!extra || (p->extra_w && p->extra_b), "%s: null extra_conv %s", who, what);
  for (int i = 0; i < n_dil; ++i) MI_CHECK_ARG(p->br_w[i] && p->br_b[i], "%s: null %s of branch %d", who, what, i);
  return MI_OK;
}
template <typename P>
static mi_dilgate_params db_branches(const P* p) {
  mi_dilgate_params q;
  for (int i = 0; i < DG_MAX_N; ++i) { q.w[i] = p->br_w[i]; q.b[i] = p->br_b[i]; }
  return q;
}
template <typename G>
static mi_dilgate_grads db_branch_grads(const G* g) {
  mi_dilgate_grads q;
  for (int i = 0; i < DG_MAX_N; ++i) { q.w[i] = g->br_w[i]; q.b[i] = g->br_b[i]; }
  q.accumulate = g->accumulate;
  return q;
}

// ------------------------------------------------------------------ DBlock: layouts
struct DbSaved {
  GhSaved gh;
  void* y0; void* u; void* h;
  float* mean2; float* rstd2; float* M5; float* b5f; float* M5s; float* M5ts;
  size_t bytes;
};
// train: everything the backward reads; inference (in the workspace): the same planes, nothing outlives the call
static DbSaved db_saved_layout(const mi_dblock_shape* s, void* base) {
  const size_t B = s->B, C = s->C, N = (size_t)s->H * s->W, cc = B * C * C;
  const int dt = s->dtype;
  Carver cv(base);
  DbSaved r;
  r.gh = gh_saved_carve(cv, s, false, s->extra != 0);
  r.y0 = cv.take(tbytes(B * C * N, dt));
  r.u = cv.take(tbytes(B * 2 * C * N, dt));
  r.h = cv.take(tbytes(B * C * N, dt));
  r.mean2 = cv.take<float>(fbytes(B * N));
  r.rstd2 = cv.take<float>(fbytes(B * N));
  r.M5 = cv.take<float>(fbytes(cc));
  r.b5f = cv.take<float>(fbytes(C));
  r.M5s = cv.take<float>(fbytes(2 * cc));
  r.M5ts = cv.take<float>(fbytes(2 * cc));
  r.bytes = cv.off;
  return r;
}

struct DbWs { GhWs gh; void* pc_ws; DbSaved inf; size_t bytes; };
static DbWs db_ws_layout(const mi_dblock_shape* s, void* base, int R) {
  Carver cv(base);
  DbWs w;
  // (conv5's Gram is summed over the batch)
  w.gh = gh_ws_carve(cv, s, R, gram_ws_bytes(probe_wgrad(s->C, s->C, s->B, (int64_t)s->H * s->W, s->dtype, 1)));
  w.pc_ws = cv.take(fbytes(pc_part_floats(s->B, s->C, s->H, s->W)));
  w.inf = db_saved_layout(s, ws_at(base, cv.off));
  w.bytes = cv.off + gh_ws_tail(w.gh, ws_at(base, cv.off), w.inf.bytes, s);
  return w;
}

static int db_check(const mi_dblock_shape* s, int* R) {
  MI_CHECK_ARG(s, "dblock: null shape");
  MI_CHECK_ARG(s->C <= DB_MAX_C, "dblock: C=%d not covered (C <= %d)", s->C, DB_MAX_C);
  MI_TRY(dg_check(s->B, s->C, s->H, s->W, s->n_dil, s->dil, s->dtype, R));
  MI_CHECK_ARG((int64_t)2 * s->C * s->H * s->W < (1ll << 31), "dblock: 2*C*H*W must be below 2^31");
  return MI_OK;
}
template <typename P>   // P = mi_dblock_params or mi_dblock_grads
static int db_check_par(const char* who, const char* what, const mi_dblock_shape* s, const P* p) {
  MI_CHECK_ARG(p, "%s: null %s", who, what);
  return gh_check_par(who, what, p, p->norm2_w && p->norm2_b && p->conv4_w && p->conv4_b && p->conv5_w && p->conv5_b && p->gamma, s->extra,
                      s->n_dil);
}

static int db_fold(const float* pool, const float* wsca, const float* bsca, const float* w, const float* bias, const float* scale, float* s_out,
                   float* M, float* Ms, float* Mts, float* bias_out, int B, int C, int64_t N, hipStream_t st) {
  ProfScope ps(st, K_DK_FOLD, 4.0 * C * C * (1.0 + 2.0 * B), 2.0 * C * C * (1.0 + B));
  hipLaunchKernelGGL(dk_fold_kernel, dim3(B), dim3(256), 2 * C * sizeof(float), st, pool, wsca, bsca, w, bias, scale, s_out, M, Ms,
                     Mts, bias_out, C, 1.0f / (float)N);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
static int db_split(const float* w, float* out, int M, int K, bool transpose, hipStream_t st) {
  ProfScope ps(st, K_DK_FOLD, 12.0 * M * K, 2.0 * M * K);
  hipLaunchKernelGGL(dk_split_kernel, dim3(cdiv_cap((int64_t)M * K, 256, 256)), dim3(256), 0, st, w, out, M, K, transpose ? 1 : 0);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
// y = W x + bias of a static 1x1 conv, w [M][K]; bf16: through the split image (scratch: 2 M K floats)
static int db_conv(const void* x, int K, const float* w, const float* bias, void* y, int M, int B, int64_t N, int dt, float* scratch,
                   void* pw_ws, hipStream_t st) {
  const bool sp = dt == MI_BF16;
  if (sp) MI_TRY(db_split(w, scratch, M, K, false, st));
  const mi_pw_desc d = db_gemm(x, K, sp ? scratch : w, sp, false, bias, nullptr, y, M, B, N, dt);
  return mi_pw_gemm(&d, pw_ws, st);
}
// backward of that conv: dw (+)= sum_b dy x^T, db (+)= sum dy, dx = W^T dy (bf16: the transposed split image)
static int db_conv_bwd(const void* dy, int M, const void* x, int K, const float* w, float* dw, float* db, void* dx, int B, int64_t N, int dt,
                       int acc, float* scratch, void* gram_ws, void* cs_ws, void* pw_ws, hipStream_t st) {
  if (dt != MI_BF16) return conv1x1_bwd_input(dy, M, x, K, w, dw, db, dx, B, N, dt, acc, gram_ws, cs_ws, pw_ws, st, false);
  const mi_gram_desc g = wgrad_gram(dy, M, x, K, B, N, dt, dw, acc);
  MI_TRY(mi_gram(&g, gram_ws, st));
  MI_TRY(launch_chan_sum(dy, db, B, M, N, dt, acc, cs_ws, st));
  MI_TRY(db_split(w, scratch, M, K, true, st));
  const mi_pw_desc d = db_gemm(dy, M, scratch, true, false, nullptr, nullptr, dx, K, B, N, dt);
  return mi_pw_gemm(&d, pw_ws, st);
}

// ------------------------------------------------------------------ the gated half: forward and backward
// y = inp + M3[b] g + b3f from inp (arch_model.py:118-129 and :183-193).  extra() runs the block's extra_conv, at the place the
// storage gives it: x0 -> cin in front of conv1, or x1 -> gin behind it (never both: a block has one extra_conv, so one callable).
template <typename S, typename P, typename Extra>
static int gh_fwd(const S* s, const P* p, const void* inp, const GhSaved& sv, const GhWs& w, hipStream_t st, Extra extra) {
  const int B = s->B, C = s->C, dt = s->dtype;
  const int64_t N = (int64_t)s->H * s->W;
  const bool b16 = dt == MI_BF16;
  MI_TRY(mi_ln_fwd_eps(inp, p->norm1_w, p->norm1_b, sv.x0, sv.mean1, sv.rstd1, B, C, N, 1, 1e-6f, dt, st));
  if (sv.cin != sv.x0) MI_TRY(extra());
  MI_TRY(db_conv(sv.cin, C, p->conv1_w, p->conv1_b, sv.x1, 2 * C, B, N, dt, w.wsplit, w.pw_ws, st));
  if (sv.gin != sv.x1) MI_TRY(extra());
  const mi_dilgate_params br = db_branches(p);
  MI_TRY(launch_dilgate_fwd(sv.gin, &br, sv.g, sv.pool, B, C, s->H, s->W, s->n_dil, s->dil, dt, w.dg_fwd_ws, st));
  MI_TRY(db_fold(sv.pool, p->sca_w, p->sca_b, p->conv3_w, p->conv3_b, p->beta, sv.s, sv.M3, b16 ? sv.M3s : nullptr, b16 ? sv.M3ts : nullptr,
                 sv.b3f, B, C, N, st));
  mi_pw_desc d3 = db_gemm(sv.g, C, b16 ? sv.M3s : sv.M3, b16, true, sv.b3f, inp, sv.y, C, B, N, dt);
  return mi_pw_gemm(&d3, w.pw_ws, st);
}

// dinp and the chain's parameter gradients from the whole gradient at y, which the block's second half left in w.t3.  w.t1 and
// w.t2 are a ping-pong: a plane is written only once its content is dead, and on entry both hold dead planes of the second half
// (t1: the gradient at norm2's output; t2: DBlock's du, EBlock's dyr).  extra(d_out, d_in) is extra_conv's backward.
template <typename S, typename P, typename G, typename Extra>
static int gh_bwd(const S* s, const P* p, const G* g, const void* inp, void* dinp, const GhSaved& sv, const GhWs& w, hipStream_t st,
                  Extra extra) {
  const int B = s->B, C = s->C, dt = s->dtype, acc = g->accumulate;
  const int64_t N = (int64_t)s->H * s->W;
  const bool b16 = dt == MI_BF16;
  const float inv_n = 1.0f / (float)N;
  const void* dy = w.t3;
  mi_gram_desc g3 = wgrad_gram(dy, C, sv.g, C, B, N, dt, w.G, 0, 0);
  MI_TRY(mi_gram(&g3, w.gram_ws, st));
  MI_TRY(launch_chan_sum(dy, w.S, 1, B * C, N, dt, 0, w.cs_ws, st));       // per image: [B][c]
  {
    ProfScope ps(st, K_DK_FOLD_BWD, 4.0 * (2.0 * B + 3) * C * C, 2.0 * (3.0 * B + 2) * C * C);
    hipLaunchKernelGGL(dk_sca_ds_kernel, dim3(B), dim3(256), C * sizeof(float), st, w.G, p->conv3_w, p->beta, p->sca_w, w.ds, w.dg_add, C, inv_n);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(dk_fold_bwd_kernel, dim3(C), dim3(256), 0, st, w.G, sv.s, w.S, p->conv3_w, p->conv3_b, p->beta, g->conv3_w, g->conv3_b,
                       g->beta, B, C, acc);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(dk_sca_w_kernel, dim3(C), dim3(256), 0, st, w.ds, sv.pool, g->sca_w, g->sca_b, B, C, inv_n, acc);
    MI_LAUNCH_CHECK();
  }
  void* dgp = w.t1;    // (the gradient at norm2's output is dead)
  mi_pw_desc e3 = b16 ? db_gemm(dy, C, sv.M3ts, true, true, nullptr, nullptr, dgp, C, B, N, dt) : db_gemm_t(dy, C, sv.M3, true, dgp, C, B, N, dt);
  MI_TRY(mi_pw_gemm(&e3, w.pw_ws, st));
  const mi_dilgate_params br = db_branches(p);
  const mi_dilgate_grads bg = db_branch_grads(g);
  void* cur = w.t2;    // (du / dyr is dead) the gradient at the gate's input
  void* dead = w.t1;   // (dg is dead once the gate's backward returns)
  MI_TRY(launch_dilgate_bwd(dgp, w.dg_add, sv.gin, &br, cur, &bg, B, C, s->H, s->W, s->n_dil, s->dil, dt, w.dg_bwd_ws, st));
  if (sv.gin != sv.x1) { MI_TRY(extra(cur, dead)); std::swap(cur, dead); }     // -> the gradient at x1 (the one at the gate's input is dead)
  MI_TRY(db_conv_bwd(cur, 2 * C, sv.cin, C, p->conv1_w, g->conv1_w, g->conv1_b, dead, B, N, dt, acc, w.wsplit, w.gram_ws, w.cs_ws, w.pw_ws, st));
  std::swap(cur, dead);      // the gradient at conv1's input (the one at x1 is dead)
  if (sv.cin != sv.x0) { MI_TRY(extra(cur, dead)); std::swap(cur, dead); }     // -> the gradient at x0
  return mi_ln_bwd(cur, inp, p->norm1_w, sv.mean1, sv.rstd1, dy, dinp, g->norm1_w, g->norm1_b, B, C, N, 1, acc, dt, w.ln_ws, st);
}

// ------------------------------------------------------------------ EBlock's tail: out = y (1 + gamma f)
// Streaming kernels, grid (S, C, B): the workgroups (.., c, b) share plane (b, c), whose N elements are a scalar head up to the first
// 16-byte boundary (`a0`: the element offset of the tensors' base inside its 16-byte line, the same for every tensor of a call),
// nv vectors of V elements dealt to the S workgroups in turn (vector v to workgroup v / 256 mod S), and a scalar tail; workgroup 0
// takes head and tail.  gamma[c] is one scalar load per workgroup: no index arithmetic per element.
constexpr int FG_ITER = 4, FG_MAX_S = 64;
template <typename T> struct FgVec { static constexpr int V = 16 / sizeof(T); };
struct FgSpan { int64_t base; int head, tail; int64_t nv; };
template <int V>
__device__ __forceinline__ FgSpan fg_span(int64_t plane, int64_t N, int a0) {
  FgSpan s;
  s.base = plane * N;
  const int mis = (int)((s.base + a0) % V);
  const int64_t h = mis ? V - mis : 0;
  s.head = (int)(h < N ? h : N);
  s.nv = (N - s.head) / V;
  s.tail = (int)(N - s.head - s.nv * V);
  return s;
}
static int fg_slices(int64_t N, int dtype) { return cdiv_cap(N, (int64_t)256 * (16 / dtype_size(dtype)) * FG_ITER, FG_MAX_S); }

template <typename T, int V>
__global__ __launch_bounds__(256) void fregate_fwd_kernel(const T* __restrict__ y, const T* __restrict__ f, const float* __restrict__ gamma,
                                                          T* __restrict__ out, int64_t N, int a0) {
  const int c = blockIdx.y, C = gridDim.y;
  const FgSpan sp = fg_span<V>((int64_t)blockIdx.z * C + c, N, a0);
  const float gm = gamma[c];
  const int64_t body = sp.base + sp.head;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < sp.nv; v += (int64_t)gridDim.x * 256) {
    float yy[V], ff[V], o[V];
    Vec<T, V>::ld(y + body + v * V, yy);
    Vec<T, V>::ld(f + body + v * V, ff);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = yy[i] * fmaf(gm, ff[i], 1.0f);
    Vec<T, V>::st(out + body + v * V, o);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < sp.head + sp.tail) {
    const int t = threadIdx.x;
    const int64_t e = sp.base + (t < sp.head ? t : sp.head + sp.nv * V + (t - sp.head));
    st1(out + e, ld1(y + e) * fmaf(gm, ld1(f + e), 1.0f));
  }
}

// part[(b S + blockIdx.x) C + c] = this workgroup's share of sum_p dout y f (its threads' sums, then the 4 waves in order)
template <typename T, int V>
__global__ __launch_bounds__(256) void fregate_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ y, const T* __restrict__ f,
                                                          const float* __restrict__ gamma, T* __restrict__ df, T* __restrict__ dyr,
                                                          float* __restrict__ part, int64_t N, int a0) {
  __shared__ float red[4];
  const int c = blockIdx.y, C = gridDim.y;
  const FgSpan sp = fg_span<V>((int64_t)blockIdx.z * C + c, N, a0);
  const float gm = gamma[c];
  const int64_t body = sp.base + sp.head;
  float acc = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < sp.nv; v += (int64_t)gridDim.x * 256) {
    float dd[V], yy[V], ff[V], o1[V], o2[V];
    Vec<T, V>::ld(dout + body + v * V, dd);
    Vec<T, V>::ld(y + body + v * V, yy);
    Vec<T, V>::ld(f + body + v * V, ff);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      o1[i] = (dd[i] * gm) * yy[i];
      o2[i] = dd[i] * fmaf(gm, ff[i], 1.0f);
      acc = fmaf(dd[i] * yy[i], ff[i], acc);
    }
    Vec<T, V>::st(df + body + v * V, o1);
    Vec<T, V>::st(dyr + body + v * V, o2);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < sp.head + sp.tail) {
    const int t = threadIdx.x;
    const int64_t e = sp.base + (t < sp.head ? t : sp.head + sp.nv * V + (t - sp.head));
    const float d = ld1(dout + e), yv = ld1(y + e), fv = ld1(f + e);
    st1(df + e, (d * gm) * yv);
    st1(dyr + e, d * fmaf(gm, fv, 1.0f));
    acc = fmaf(d * yv, fv, acc);
  }
  const float s = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    part[((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * C + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

static int fg_check(const char* who, int B, int C, int64_t N, int dtype) {
  MI_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && C <= 65535 && N > 0, "%s: bad shape B=%d C=%d N=%lld", who, B, C, (long long)N);
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "%s: bad dtype %d", who, dtype);
  MI_CHECK_ARG((int64_t)B * C <= ((int64_t)1 << 62) / N, "%s: tensor too large", who);
  return MI_OK;
}
// the element offset inside a 16-byte line that every pointer shares, or -1 (the scalar form)
static int fg_a0(std::initializer_list<const void*> ps, int dtype) {
  const uintptr_t first = reinterpret_cast<uintptr_t>(*ps.begin()) & 15u;
  for (const void* p : ps)
    if ((reinterpret_cast<uintptr_t>(p) & 15u) != first) return -1;
  return first % dtype_size(dtype) ? -1 : (int)(first / dtype_size(dtype));
}

static int launch_fregate_fwd(const void* y, const void* f, const float* gamma, void* out, int B, int C, int64_t N, int dtype,
                              hipStream_t st) {
  MI_TRY(fg_check("fregate_fwd", B, C, N, dtype));
  MI_CHECK_ARG(y && f && gamma && out, "fregate_fwd: null pointer");
  const int a0 = fg_a0({y, f, out}, dtype);
  const dim3 grid(fg_slices(N, dtype), C, B);
  const double n = (double)B * C * N;
  ProfScope ps(st, K_EWISE, 3.0 * n * dtype_size(dtype), 3.0 * n);
  return with_dtype(dtype, "fregate_fwd", [&](auto tag) {
    using T = decltype(tag);
    if (a0 >= 0)
      hipLaunchKernelGGL((fregate_fwd_kernel<T, FgVec<T>::V>), grid, dim3(256), 0, st, (const T*)y, (const T*)f, gamma, (T*)out, N, a0);
    else
      hipLaunchKernelGGL((fregate_fwd_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)y, (const T*)f, gamma, (T*)out, N, 0);
  });
}

static size_t fg_bwd_ws(int B, int C, int64_t N) { return fbytes((size_t)B * FG_MAX_S * C); }

static int launch_fregate_bwd(const void* dout, const void* y, const void* f, const float* gamma, void* df, void* dyr, float* dgamma,
                              int B, int C, int64_t N, int accumulate, int dtype, void* ws, hipStream_t st) {
  MI_TRY(fg_check("fregate_bwd", B, C, N, dtype));
  MI_CHECK_ARG(dout && y && f && gamma && df && dyr && dgamma && ws, "fregate_bwd: null pointer");
  const int a0 = fg_a0({dout, y, f, df, dyr}, dtype);
  const int S = fg_slices(N, dtype);
  const dim3 grid(S, C, B);
  float* part = (float*)ws;
  {
    const double n = (double)B * C * N;
    ProfScope ps(st, K_EWISE, 5.0 * n * dtype_size(dtype), 8.0 * n);
    MI_TRY(with_dtype(dtype, "fregate_bwd", [&](auto tag) {
      using T = decltype(tag);
      if (a0 >= 0)
        hipLaunchKernelGGL((fregate_bwd_kernel<T, FgVec<T>::V>), grid, dim3(256), 0, st, (const T*)dout, (const T*)y, (const T*)f, gamma,
                           (T*)df, (T*)dyr, part, N, a0);
      else
        hipLaunchKernelGGL((fregate_bwd_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)dout, (const T*)y, (const T*)f, gamma, (T*)df,
                           (T*)dyr, part, N, 0);
    }));
  }
  return launch_reduce_rows(part, dgamma, (int64_t)B * S, C, C, accumulate, 1.0f, st);
}

// ------------------------------------------------------------------ EBlock: layouts
struct EbSaved {
  GhSaved gh;
  void* f; float* mean2; float* rstd2; void* blob;
  size_t sec[9];     // bytes of x0, xe, x1, g, y, f, the statistics, the small tensors, the FreMLP blob
  size_t bytes;
};
static mi_fremlp_shape eb_fre_shape(const mi_eblock_shape* s) { return mi_fremlp_shape{s->B, s->C, 2, s->H, s->W, s->dtype}; }
// train: everything the backward reads; inference (blob = false, in the workspace): the same planes, nothing outlives the call
static EbSaved eb_saved_layout(const mi_eblock_shape* s, void* base, bool blob) {
  const size_t N = (size_t)s->H * s->W;
  Carver cv(base);
  EbSaved r;
  r.gh = gh_saved_carve(cv, s, s->extra != 0, false);
  const size_t* gs = r.gh.sec;      // x0, xe, x1, (no plane behind conv1,) g, y, mean1 / rstd1, the small tensors
  size_t o = cv.off, own[3];        // f, mean2 / rstd2, the FreMLP blob
  auto close = [&](int i) { own[i] = cv.off - o; o = cv.off; };
  r.f = cv.take(tbytes(s->B * s->C * N, s->dtype)); close(0);
  r.mean2 = cv.take<float>(fbytes(s->B * N));
  r.rstd2 = cv.take<float>(fbytes(s->B * N)); close(1);
  const mi_fremlp_shape fs = eb_fre_shape(s);
  r.blob = blob ? cv.take(mi_fremlp_saved_bytes(&fs)) : nullptr; close(2);
  r.bytes = cv.off;
  const size_t sec[9] = {gs[0], gs[1], gs[2], gs[4], gs[5], own[0], gs[6] + own[1], gs[7], own[2]};
  memcpy(r.sec, sec, sizeof(sec));
  return r;
}

struct EbWs { GhWs gh; void* dw_ws; void* fre_ws; void* fg_ws; void* y0; EbSaved inf; size_t bytes; };
static EbWs eb_ws_layout(const mi_eblock_shape* s, void* base, int R) {
  Carver cv(base);
  EbWs w;
  w.gh = gh_ws_carve(cv, s, R, 0);
  w.dw_ws = cv.take(s->extra ? mi_dwconv_bwd_workspace(s->B, s->C, s->H, s->W, 3) : 0);
  const mi_fremlp_shape fs = eb_fre_shape(s);
  w.fre_ws = cv.take(mi_fremlp_workspace(&fs));
  w.fg_ws = cv.take(fg_bwd_ws(s->B, s->C, (int64_t)s->H * s->W));
  w.y0 = cv.take(tbytes((size_t)s->B * s->C * s->H * s->W, s->dtype));       // LayerNorm2d(y): FreMLP's input, dead when the forward returns
  w.inf = eb_saved_layout(s, ws_at(base, cv.off), false);
  w.bytes = cv.off + gh_ws_tail(w.gh, ws_at(base, cv.off), w.inf.bytes, s);
  return w;
}

constexpr int EB_MIN_HW = 2, EB_MAX_HW = 512;
static int eb_check(const mi_eblock_shape* s, int* R) {
  MI_CHECK_ARG(s, "eblock: null shape");
  MI_CHECK_ARG(s->C >= 1 && s->C <= DB_MAX_C, "eblock: C=%d not covered (1 <= C <= %d)", s->C, DB_MAX_C);
  MI_CHECK_ARG(s->H >= EB_MIN_HW && s->H <= EB_MAX_HW && s->W >= EB_MIN_HW && s->W <= EB_MAX_HW,
               "eblock: plane %d x %d not covered (%d <= H, W <= %d: FreMLP's dense transforms)", s->H, s->W, EB_MIN_HW, EB_MAX_HW);
  MI_TRY(dg_check(s->B, s->C, s->H, s->W, s->n_dil, s->dil, s->dtype, R));
  MI_CHECK_ARG((int64_t)2 * s->C * s->H * s->W < (1ll << 31), "eblock: 2*C*H*W must be below 2^31");
  const mi_fremlp_shape fs = eb_fre_shape(s);
  if (mi_fremlp_workspace(&fs) == 0) return MI_ERR_ARG;      // (its message stands)
  return MI_OK;
}
template <typename P>   // P = mi_eblock_params or mi_eblock_grads
static int eb_check_par(const char* who, const char* what, const mi_eblock_shape* s, const P* p) {
  MI_CHECK_ARG(p, "%s: null %s", who, what);
  return gh_check_par(who, what, p, p->norm2_w && p->norm2_b && p->fre_w1 && p->fre_b1 && p->fre_w2 && p->fre_b2 && p->gamma, s->extra,
                      s->n_dil);
}

}  // namespace mi

using namespace mi;

extern "C" int mi_dilgate_plan(int B, int c, int H, int W, int dtype, int n_dil, const int* dil, int64_t* out) {
  MI_CHECK_ARG(out, "dilgate_plan: null pointer");
  int R = 0;
  MI_TRY(dg_check(B, c, H, W, n_dil, dil, dtype, &R));
  const DgPlan p = dg_plan(B, c, H, W, n_dil, R, dtype);
  const int64_t v[12] = {p.th, p.tw, p.R, (int64_t)p.lds, p.tiles, c, B, p.tiles, 0, (int64_t)p.fwd_ws, p.splits, (int64_t)p.bwd_ws};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
  return MI_OK;
}
extern "C" size_t mi_dilgate_fwd_workspace(int B, int c, int H, int W) {
  const int one = 1;
  int R = 0;
  if (dg_check(B, c, H, W, 1, &one, MI_F32, &R) != MI_OK) return 0;
  return dg_plan(B, c, H, W, 1, 1, MI_F32).fwd_ws;
}
extern "C" int mi_dilgate_fwd(const void* x, const mi_dilgate_params* p, void* g, float* pool, int B, int c, int H, int W, int n_dil,
                              const int* dil, int dtype, void* ws, void* stream) {
  return launch_dilgate_fwd(x, p, g, pool, B, c, H, W, n_dil, dil, dtype, ws, (hipStream_t)stream);
}
extern "C" size_t mi_dilgate_bwd_workspace(int B, int c, int H, int W, int n_dil, int dtype) {
  const int ones[DG_MAX_N] = {1, 1, 1, 1};
  int R = 0;
  if (dg_check(B, c, H, W, n_dil, ones, dtype, &R) != MI_OK) return 0;
  return dg_plan(B, c, H, W, n_dil, 1, dtype).bwd_ws;
}
extern "C" int mi_dilgate_bwd(const void* dg, const float* dg_add, const void* x, const mi_dilgate_params* p, void* dx,
                              const mi_dilgate_grads* gr, int B, int c, int H, int W, int n_dil, const int* dil, int dtype, void* ws,
                              void* stream) {
  return launch_dilgate_bwd(dg, dg_add, x, p, dx, gr, B, c, H, W, n_dil, dil, dtype, ws, (hipStream_t)stream);
}
extern "C" int mi_pairconv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int c, int H, int W, int dtype,
                                  void* stream) {
  return launch_pairconv<1>(x, w, bias, y, B, c, H, W, dtype, (hipStream_t)stream);
}
extern "C" size_t mi_pairconv3x3_bwd_workspace(int B, int c, int H, int W) {
  if (pc_check(B, c, H, W, MI_F32) != MI_OK) return 0;
  return fbytes(pc_part_floats(B, c, H, W));
}
extern "C" int mi_pairconv3x3_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, int B, int c, int H,
                                  int W, int accumulate, int dtype, void* ws, void* stream) {
  return launch_pairconv_bwd(dy, x, w, dx, dw, db, B, c, H, W, accumulate, dtype, ws, (hipStream_t)stream);
}

extern "C" size_t mi_dblock_saved_bytes(const mi_dblock_shape* s) {
  int R = 0;
  if (db_check(s, &R) != MI_OK) return 0;
  return db_saved_layout(s, nullptr).bytes;
}
extern "C" size_t mi_dblock_workspace(const mi_dblock_shape* s) {
  int R = 0;
  if (db_check(s, &R) != MI_OK) return 0;
  return db_ws_layout(s, nullptr, R).bytes;
}

extern "C" int mi_dblock_fwd(const mi_dblock_shape* s, const mi_dblock_params* p, const void* inp, void* out, void* saved, void* ws,
                             void* stream) {
  int R = 0;
  MI_TRY(db_check(s, &R));
  MI_TRY(db_check_par("dblock", "parameter", s, p));
  MI_CHECK_ARG(inp && out && ws, "dblock_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype;
  const int64_t N = (int64_t)H * W;
  const bool b16 = dt == MI_BF16;
  const DbWs ws_ = db_ws_layout(s, ws, R);
  const GhWs& w = ws_.gh;
  const DbSaved sv = saved ? db_saved_layout(s, saved) : ws_.inf;
  // first half (arch_model.py:118-129)
  MI_TRY(gh_fwd(s, p, inp, sv.gh, w, st,
                [&] { return launch_pairconv<1>(sv.gh.x1, p->extra_w, p->extra_b, sv.gh.gin, B, C, H, W, dt, st); }));
  // second half (:131-134)
  MI_TRY(mi_ln_fwd_eps(sv.gh.y, p->norm2_w, p->norm2_b, sv.y0, sv.mean2, sv.rstd2, B, C, N, 1, 1e-6f, dt, stream));
  MI_TRY(db_conv(sv.y0, C, p->conv4_w, p->conv4_b, sv.u, 2 * C, B, N, dt, w.wsplit, w.pw_ws, st));
  const size_t half = (size_t)C * N * dtype_size(dt);
  MI_TRY(mi_ewise_fwd(sv.u, 2 * C * N, (const char*)sv.u + half, 2 * C * N, sv.h, B, C * N, 0, dt, stream));
  MI_TRY(db_fold(nullptr, nullptr, nullptr, p->conv5_w, p->conv5_b, p->gamma, nullptr, sv.M5, b16 ? sv.M5s : nullptr,
                 b16 ? sv.M5ts : nullptr, sv.b5f, B, C, N, st));
  mi_pw_desc d5 = db_gemm(sv.h, C, b16 ? sv.M5s : sv.M5, b16, true, sv.b5f, sv.gh.y, out, C, B, N, dt);
  return mi_pw_gemm(&d5, w.pw_ws, stream);
}

extern "C" int mi_dblock_bwd(const mi_dblock_shape* s, const mi_dblock_params* p, const void* inp, const void* dout, void* dinp,
                             const mi_dblock_grads* g, const void* saved, void* ws, void* stream) {
  int R = 0;
  MI_TRY(db_check(s, &R));
  MI_TRY(db_check_par("dblock", "parameter", s, p));
  MI_CHECK_ARG(inp && dout && dinp && g && saved && ws, "dblock_bwd: null pointer");
  MI_TRY(db_check_par("dblock_bwd", "gradient buffer", s, g));
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype, acc = g->accumulate;
  const int64_t N = (int64_t)H * W;
  const bool b16 = dt == MI_BF16;
  const DbWs ws_ = db_ws_layout(s, ws, R);
  const GhWs& w = ws_.gh;
  const DbSaved sv = db_saved_layout(s, const_cast<void*>(saved));
  const size_t half = (size_t)C * N * dtype_size(dt);
  // ---- second half: out = y + M5 h + b5f
  void* dh = w.t1;
  mi_pw_desc e5 = b16 ? db_gemm(dout, C, sv.M5ts, true, true, nullptr, nullptr, dh, C, B, N, dt) : db_gemm_t(dout, C, sv.M5, true, dh, C, B, N, dt);
  MI_TRY(mi_pw_gemm(&e5, w.pw_ws, stream));
  mi_gram_desc g5 = wgrad_gram(dout, C, sv.h, C, B, N, dt, w.G, 0, 1);
  MI_TRY(mi_gram(&g5, w.gram_ws, stream));
  MI_TRY(launch_chan_sum(dout, w.S, B, C, N, dt, 0, w.cs_ws, st));
  {
    ProfScope ps(st, K_DK_FOLD_BWD, 4.0 * 3 * C * C, 4.0 * C * C);
    hipLaunchKernelGGL(dk_fold_bwd_kernel, dim3(C), dim3(256), 0, st, w.G, (const float*)nullptr, w.S, p->conv5_w, p->conv5_b, p->gamma,
                       g->conv5_w, g->conv5_b, g->gamma, 1, C, acc);
    MI_LAUNCH_CHECK();
  }
  void* du = w.t2;     // [B][2c]: d u1 = dh u2, d u2 = dh u1
  MI_TRY(mi_ewise_bwd(sv.u, 2 * C * N, (const char*)sv.u + half, 2 * C * N, dh, du, 2 * C * N, (char*)du + half, 2 * C * N, B, C * N, 0, dt,
                      stream));
  void* dy0 = w.t1;    // (dh is dead)
  MI_TRY(db_conv_bwd(du, 2 * C, sv.y0, C, p->conv4_w, g->conv4_w, g->conv4_b, dy0, B, N, dt, acc, w.wsplit, w.gram_ws, w.cs_ws, w.pw_ws, st));
  void* dy = w.t3;     // the whole gradient at y: through norm2 plus the residual's dout
  MI_TRY(mi_ln_bwd(dy0, sv.gh.y, p->norm2_w, sv.mean2, sv.rstd2, dout, dy, g->norm2_w, g->norm2_b, B, C, N, 1, acc, dt, w.ln_ws, stream));
  // ---- first half: y = inp + M3[b] g + b3f (dy0 and du are dead)
  return gh_bwd(s, p, g, inp, dinp, sv.gh, w, st, [&](const void* dx2, void* dx1) {
    return launch_pairconv_bwd(dx2, sv.gh.x1, p->extra_w, dx1, g->extra_w, g->extra_b, B, C, H, W, acc, dt, ws_.pc_ws, st);
  });
}

// ------------------------------------------------------------------ EBlock (arch_model.py:141-204)
extern "C" int mi_fregate_fwd(const void* y, const void* f, const float* gamma, void* out, int B, int C, int64_t N, int dtype,
                              void* stream) {
  return launch_fregate_fwd(y, f, gamma, out, B, C, N, dtype, (hipStream_t)stream);
}
extern "C" size_t mi_fregate_bwd_workspace(int B, int C, int64_t N) {
  if (fg_check("fregate_bwd_workspace", B, C, N, MI_F32) != MI_OK) return 0;
  return fg_bwd_ws(B, C, N);
}
extern "C" int mi_fregate_bwd(const void* dout, const void* y, const void* f, const float* gamma, void* df, void* dyr, float* dgamma,
                              int B, int C, int64_t N, int accumulate, int dtype, void* ws, void* stream) {
  return launch_fregate_bwd(dout, y, f, gamma, df, dyr, dgamma, B, C, N, accumulate, dtype, ws, (hipStream_t)stream);
}

extern "C" size_t mi_eblock_saved_bytes(const mi_eblock_shape* s) {
  int R = 0;
  if (eb_check(s, &R) != MI_OK) return 0;
  return eb_saved_layout(s, nullptr, true).bytes;
}
extern "C" size_t mi_eblock_workspace(const mi_eblock_shape* s) {
  int R = 0;
  if (eb_check(s, &R) != MI_OK) return 0;
  return eb_ws_layout(s, nullptr, R).bytes;
}
extern "C" int mi_eblock_plan(const mi_eblock_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "eblock_plan: null pointer");
  int R = 0;
  MI_TRY(eb_check(s, &R));
  const EbSaved sv = eb_saved_layout(s, nullptr, true);
  const EbWs w = eb_ws_layout(s, nullptr, R);
  const mi_fremlp_shape fs = eb_fre_shape(s);
  int64_t fp[64];
  MI_TRY(mi_fremlp_plan(&fs, fp));
  const int b16 = s->dtype == MI_BF16 ? 1 : 0, ex = s->extra ? 1 : 0, n = s->n_dil;
  // forward: norm1, [extra_conv], conv1 (bf16: the split first), the gate and its pool sum, the fold, conv3, norm2, FreMLP, the tail
  const int64_t fwd = 1 + ex + (1 + b16) + 2 + 1 + 1 + 1 + (fp[18] + fp[20]) + 1;
  // backward: the tail and its row sum, FreMLP, norm2; Gram, channel sums, three c x c kernels, conv3^T; the gate's two passes and
  // 2n row sums; conv1 (Gram, channel sum, [split], product); [extra_conv and its two row sums]; norm1
  const int64_t bwd = 2 + (fp[19] + fp[21]) + 1 + 2 + 3 + 1 + (2 + 2 * n) + (3 + b16) + 3 * ex + 1;
  for (int i = 0; i < 9; ++i) out[i] = (int64_t)sv.sec[i];
  out[9] = (int64_t)sv.bytes;
  out[10] = (int64_t)w.bytes;
  out[11] = fwd;
  out[12] = bwd;
  out[13] = fg_slices((int64_t)s->H * s->W, s->dtype);
  out[14] = out[15] = 0;
  return MI_OK;
}

extern "C" int mi_eblock_fwd(const mi_eblock_shape* s, const mi_eblock_params* p, const void* inp, void* out, void* saved, void* ws,
                             void* stream) {
  int R = 0;
  MI_TRY(eb_check(s, &R));
  MI_TRY(eb_check_par("eblock", "parameter", s, p));
  MI_CHECK_ARG(inp && out && ws, "eblock_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype;
  const int64_t N = (int64_t)H * W;
  const EbWs w = eb_ws_layout(s, ws, R);
  const EbSaved sv = saved ? eb_saved_layout(s, saved, true) : w.inf;
  // first half (arch_model.py:183-193)
  MI_TRY(gh_fwd(s, p, inp, sv.gh, w.gh, st,
                [&] { return mi_dwconv_fwd(sv.gh.x0, p->extra_w, p->extra_b, sv.gh.cin, B, C, H, W, 3, dt, stream); }));
  // second half (:196-199)
  MI_TRY(mi_ln_fwd_eps(sv.gh.y, p->norm2_w, p->norm2_b, w.y0, sv.mean2, sv.rstd2, B, C, N, 1, 1e-6f, dt, stream));
  const mi_fremlp_shape fs = eb_fre_shape(s);
  MI_TRY(mi_fremlp_fwd(&fs, p->fre_w1, p->fre_b1, p->fre_w2, p->fre_b2, w.y0, sv.f, saved ? sv.blob : nullptr, w.fre_ws, stream));
  return launch_fregate_fwd(sv.gh.y, sv.f, p->gamma, out, B, C, N, dt, st);
}

extern "C" int mi_eblock_bwd(const mi_eblock_shape* s, const mi_eblock_params* p, const void* inp, const void* dout, void* dinp,
                             const mi_eblock_grads* g, const void* saved, void* ws, void* stream) {
  int R = 0;
  MI_TRY(eb_check(s, &R));
  MI_TRY(eb_check_par("eblock", "parameter", s, p));
  MI_CHECK_ARG(inp && dout && dinp && g && saved && ws, "eblock_bwd: null pointer");
  MI_TRY(eb_check_par("eblock_bwd", "gradient buffer", s, g));
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype, acc = g->accumulate;
  const int64_t N = (int64_t)H * W;
  const EbWs w = eb_ws_layout(s, ws, R);
  const EbSaved sv = eb_saved_layout(s, const_cast<void*>(saved), true);
  // ---- second half: out = y (1 + gamma f), f = FreMLP(LN(y))
  void* df = w.gh.t3;
  void* dyr = w.gh.t2;    // the residual's share of the gradient at y
  MI_TRY(launch_fregate_bwd(dout, sv.gh.y, sv.f, p->gamma, df, dyr, g->gamma, B, C, N, acc, dt, w.fg_ws, st));
  void* dy0 = w.gh.t1;
  const mi_fremlp_shape fs = eb_fre_shape(s);
  MI_TRY(mi_fremlp_bwd(&fs, p->fre_w1, p->fre_w2, p->fre_b2, df, dy0, g->fre_w1, g->fre_b1, g->fre_w2, g->fre_b2, acc, sv.blob, w.fre_ws,
                       stream));
  void* dy = w.gh.t3;     // (df is dead) the whole gradient at y: through norm2 plus the residual's share
  MI_TRY(mi_ln_bwd(dy0, sv.gh.y, p->norm2_w, sv.mean2, sv.rstd2, dyr, dy, g->norm2_w, g->norm2_b, B, C, N, 1, acc, dt, w.gh.ln_ws, stream));
  // ---- first half: y = inp + M3[b] g + b3f (dy0 and dyr are dead)
  return gh_bwd(s, p, g, inp, dinp, sv.gh, w.gh, st, [&](const void* dxe, void* dx0) {
    return mi_dwconv_bwd(dxe, sv.gh.x0, p->extra_w, dx0, g->extra_w, g->extra_b, B, C, H, W, 3, acc, dt, w.dw_ws, stream);
  });
}
