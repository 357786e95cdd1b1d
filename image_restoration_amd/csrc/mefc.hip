// DRSformer's Mixture of Experts Feature Compensator (MEFC, `subnet`, DRSformer_arch.py:328-354): one OALayer routing head plus
// the GroupOLs it weights (:206-247), forward and backward, as one C-ABI unit (mi_mefc_*).
//
// Per step t the eight operations of OperationLayer (:189-204) all end in a linear map and the routing weight w_i[b] is a scalar
// per image, so the out projection, each op's trailing 1x1 and w_i[b] fold into one per-image matrix (MDTA's softmax fold):
//   pre[b] = M[b] . Z[b],   M[b][:, iC:(i+1)C] = w_i[b] . out_w[:, iC:(i+1)C] . pw_i   (pw_7 = I: the average pool)
//   Z = [z_sep1, z_sep3, z_sep5, z_sep7, dil3(s), dil5(s), dil7(s), avg(s)]            (8C planes; the concatenation never exists)
//   z_sep_k = dw2_k(relu(U_k)),  U_k = pw1_k . D1_k,  D1_k = dw1_k(s)
// Launches per step: stencil A (one read of s with a 6-pixel halo -> D1 [4C] and Z panels 4..7), four pw1 GEMMs, stencil B
// (relu as the tile is loaded, dw2_k -> Z panels 0..3), the fold (M in fp32 and bf16, both orientations), the per-image GEMM
// over K = 8C, and the residual epilogue s' = relu(relu(pre) + s).
// Backward: G[b] = dpre[b] Z[b]^T (per-image Gram) gives d w_i[b] = <A_i, G_i[b]>, d out_w and d pw_i (fold backward); dZ[b] =
// M[b]^T dpre[b]; the stencils' data gradients are their transposes; depthwise weight gradients are per-workgroup partial rows
// (fixed-order block sums) summed by launch_reduce_rows in a fixed order.  No float atomics: bitwise reproducible.
// Tiles of 32 x 32 output pixels, 256 threads, four rows per thread; a 6-pixel halo costs 1.9x the tile in loads (a 32 x 8 tile:
// 3.4x).  Everything is enqueued on the caller's stream; nothing reads back to the host, so a call captures into a HIP graph.
#include "internal.h"

namespace mi {

constexpr int MF_TW = 32, MF_TH = 32, MF_RPT = MF_TH / 8;   // thread (tx, ty) owns column tx, rows ty + 8 j
constexpr int MF_MAX_SPLITS = 16;                            // workgroups per (image, channel) in the weight-gradient kernels
constexpr int MF_MAX_C = 256, MF_MAX_STEPS = 16;

template <int R> struct MfTile { static constexpr int LW = MF_TW + 2 * R, LH = MF_TH + 2 * R, LT = LW * LH; };
enum { MF_PLAIN = 0, MF_RELU = 1, MF_AVG = 2 };

static inline int mf_tiles_x(int W) { return cdiv(W, MF_TW); }
static inline int mf_tiles(int H, int W) { return mf_tiles_x(W) * cdiv(H, MF_TH); }
static inline int mf_splits(int H, int W) {
  const int n = mf_tiles(H, W);
  return n < MF_MAX_SPLITS ? n : MF_MAX_SPLITS;
}

// in-plane taps of the 3x3 window at (y, x): the divisor of AvgPool2d(3, 1, 1, count_include_pad=False)
__device__ __forceinline__ float mf_cnt(int y, int x, int H, int W) {
  const int y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < H ? y + 1 : H - 1, x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < W ? x + 1 : W - 1;
  return (float)((y1 - y0 + 1) * (x1 - x0 + 1));
}

// plane tile with an R-pixel halo -> L (zero outside the plane: the convs' padding).  MF_RELU: relu(v); MF_AVG: v / count(y, x)
template <typename T, int R, int MODE>
__device__ __forceinline__ void mf_load(float* L, const T* __restrict__ p, int H, int W, int ty0, int tx0) {
  using G = MfTile<R>;
  for (int e = threadIdx.x; e < G::LT; e += 256) {
    const int ly = e / G::LW, lx = e - ly * G::LW;
    const int y = ty0 - R + ly, x = tx0 - R + lx;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      v = ld1(p + (int64_t)y * W + x);
      if (MODE == MF_RELU) v = fmaxf(v, 0.f);
      if (MODE == MF_AVG) v /= mf_cnt(y, x, H, W);
    }
    L[e] = v;
  }
}

// a[j] += sum_{dy,dx} w[dy K + dx] L[row ly + 8j + S (dy - K/2) D, column lx + S (dx - K/2) D]  (S = +1: the conv, -1: its
// transpose, i.e. the data gradient).  w == nullptr: all-ones 3x3 (the pool).
template <int K, int D, int S, int R>
__device__ __forceinline__ void mf_conv4(const float* L, const float* __restrict__ w, int ly, int lx, float (&a)[MF_RPT]) {
  constexpr int LW = MfTile<R>::LW, H2 = K / 2;
#pragma unroll
  for (int dy = 0; dy < K; ++dy)
#pragma unroll
    for (int dx = 0; dx < K; ++dx) {
      const float wv = w ? w[dy * K + dx] : 1.f;
#pragma unroll
      for (int j = 0; j < MF_RPT; ++j)
        a[j] = fmaf(wv, L[(ly + 8 * j + R + S * (dy - H2) * D) * LW + lx + R + S * (dx - H2) * D], a[j]);
    }
}

template <typename T>
__device__ __forceinline__ void mf_store4(T* __restrict__ plane, const float (&a)[MF_RPT], int H, int W, int ty0, int tx0) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, x = tx0 + tx;
#pragma unroll
  for (int j = 0; j < MF_RPT; ++j) {
    const int y = ty0 + ty + 8 * j;
    if (x < W && y < H) st1(plane + (int64_t)y * W + x, a[j]);
  }
}

__device__ __forceinline__ void mf_zero(float (&a)[MF_RPT]) {
#pragma unroll
  for (int j = 0; j < MF_RPT; ++j) a[j] = 0.f;
}

// Sums NV per-thread values over the workgroup (wave DPP sums, then the 4 waves in order); thread n < NV gets total n.
template <int NV>
__device__ __forceinline__ float mf_block_sum(const float (&v)[NV], float* red) {
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

struct MfW7 { const float* w[7]; };   // stencil A: dw1 k = 1, 3, 5, 7, then dil k = 3, 5, 7 ([C][k*k] each)
struct MfW4 { const float* w[4]; };   // stencil B: dw2 k = 1, 3, 5, 7

// ------------------------------------------------------------------ stencil A: s -> D1 (4 planes), Z panels 4..7
template <typename T>
__global__ __launch_bounds__(256) void mefc_sta_fwd_kernel(const T* __restrict__ s, MfW7 wa, T* __restrict__ d1, T* __restrict__ z,
                                                           int C, int H, int W, int tiles_x) {
  constexpr int R = 6;
  __shared__ float L[MfTile<R>::LT];
  const int ch = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * MF_TH, tx0 = (blockIdx.x % tiles_x) * MF_TW;
  const int64_t N = (int64_t)H * W, CN = (int64_t)C * N;
  mf_load<T, R, MF_PLAIN>(L, s + ((int64_t)b * C + ch) * N, H, W, ty0, tx0);
  __syncthreads();
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  T* d1b = d1 + (int64_t)b * 4 * CN + ch * N;
  T* zb = z + (int64_t)b * 8 * CN + ch * N;
  float a[MF_RPT];
  mf_zero(a); mf_conv4<1, 1, 1, R>(L, wa.w[0] + ch, ty, tx, a);      mf_store4(d1b, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<3, 1, 1, R>(L, wa.w[1] + ch * 9, ty, tx, a);  mf_store4(d1b + CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<5, 1, 1, R>(L, wa.w[2] + ch * 25, ty, tx, a); mf_store4(d1b + 2 * CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<7, 1, 1, R>(L, wa.w[3] + ch * 49, ty, tx, a); mf_store4(d1b + 3 * CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<3, 2, 1, R>(L, wa.w[4] + ch * 9, ty, tx, a);  mf_store4(zb + 4 * CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<5, 2, 1, R>(L, wa.w[5] + ch * 25, ty, tx, a); mf_store4(zb + 5 * CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<7, 2, 1, R>(L, wa.w[6] + ch * 49, ty, tx, a); mf_store4(zb + 6 * CN, a, H, W, ty0, tx0);
  mf_zero(a); mf_conv4<3, 1, 1, R>(L, nullptr, ty, tx, a);
#pragma unroll
  for (int j = 0; j < MF_RPT; ++j) {
    const int y = ty0 + ty + 8 * j, x = tx0 + tx;
    if (x < W && y < H) a[j] /= mf_cnt(y, x, H, W);
  }
  mf_store4(zb + 7 * CN, a, H, W, ty0, tx0);
}

// ds = dw1_k^T dD1_k (k = 1..7) + dil_k^T dZ_{4+k} + pool^T dZ_7 + dout (out > 0): the eight gradient planes in turn through one
// LDS tile, the residual's gradient added at the end; one write of ds.
template <typename T>
__global__ __launch_bounds__(256) void mefc_sta_bwd_kernel(const T* __restrict__ dd1, const T* __restrict__ dz, const T* __restrict__ dout,
                                                           const T* __restrict__ out, MfW7 wa, T* __restrict__ ds, int C, int H, int W,
                                                           int tiles_x) {
  constexpr int R = 6;
  __shared__ float L[MfTile<R>::LT];
  const int ch = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * MF_TH, tx0 = (blockIdx.x % tiles_x) * MF_TW;
  const int64_t N = (int64_t)H * W, CN = (int64_t)C * N;
  const T* d1b = dd1 + (int64_t)b * 4 * CN + ch * N;
  const T* zb = dz + (int64_t)b * 8 * CN + ch * N;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float a[MF_RPT];
  mf_zero(a);
#define MF_STEP(SRC, MODE, K, D, WP)                        \
  __syncthreads();                                          \
  mf_load<T, R, MODE>(L, SRC, H, W, ty0, tx0);              \
  __syncthreads();                                          \
  mf_conv4<K, D, -1, R>(L, WP, ty, tx, a);
  MF_STEP(d1b, MF_PLAIN, 1, 1, wa.w[0] + ch)
  MF_STEP(d1b + CN, MF_PLAIN, 3, 1, wa.w[1] + ch * 9)
  MF_STEP(d1b + 2 * CN, MF_PLAIN, 5, 1, wa.w[2] + ch * 25)
  MF_STEP(d1b + 3 * CN, MF_PLAIN, 7, 1, wa.w[3] + ch * 49)
  MF_STEP(zb + 4 * CN, MF_PLAIN, 3, 2, wa.w[4] + ch * 9)
  MF_STEP(zb + 5 * CN, MF_PLAIN, 5, 2, wa.w[5] + ch * 25)
  MF_STEP(zb + 6 * CN, MF_PLAIN, 7, 2, wa.w[6] + ch * 49)
  MF_STEP(zb + 7 * CN, MF_AVG, 3, 1, nullptr)
#undef MF_STEP
  const int64_t po = ((int64_t)b * C + ch) * N;
#pragma unroll
  for (int j = 0; j < MF_RPT; ++j) {
    const int y = ty0 + ty + 8 * j, x = tx0 + tx;
    if (x < W && y < H) {
      const int64_t o = po + (int64_t)y * W + x;
      const float r = ld1(out + o) > 0.f ? ld1(dout + o) : 0.f;
      st1(ds + o, a[j] + r);
    }
  }
}

// ------------------------------------------------------------------ stencil B: Z panel k = dw2_k(relu(U_k)); backward dU_k
template <typename T, int K>
__device__ __forceinline__ void mf_stb_body(float* L, const T* __restrict__ src, const float* __restrict__ w, T* __restrict__ dst,
                                            const T* __restrict__ mask, int H, int W, int ty0, int tx0) {
  constexpr int R = 3;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (mask) mf_load<T, R, MF_PLAIN>(L, src, H, W, ty0, tx0);
  else mf_load<T, R, MF_RELU>(L, src, H, W, ty0, tx0);
  __syncthreads();
  float a[MF_RPT];
  mf_zero(a);
  if (mask) mf_conv4<K, 1, -1, R>(L, w, ty, tx, a);
  else mf_conv4<K, 1, 1, R>(L, w, ty, tx, a);
#pragma unroll
  for (int j = 0; j < MF_RPT; ++j) {
    const int y = ty0 + ty + 8 * j, x = tx0 + tx;
    if (x < W && y < H) {
      const int64_t o = (int64_t)y * W + x;
      st1(dst + o, (mask && !(ld1(mask + o) > 0.f)) ? 0.f : a[j]);
    }
  }
}

// grid (tiles, 4C, B), plane k C + c.  Forward (mask == nullptr): src = U, dst = Z (panels 0..3).  Backward: src = dZ, dst = dU,
// mask = U (dU = (U > 0) dw2^T dZ).
template <typename T>
__global__ __launch_bounds__(256) void mefc_stb_kernel(const T* __restrict__ src, int64_t src_bs, MfW4 wb, T* __restrict__ dst,
                                                       int64_t dst_bs, const T* __restrict__ mask, int C, int H, int W, int tiles_x) {
  __shared__ float L[MfTile<3>::LT];
  const int k = blockIdx.y / C, ch = blockIdx.y - k * C, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * MF_TH, tx0 = (blockIdx.x % tiles_x) * MF_TW;
  const int64_t N = (int64_t)H * W, pl = ((int64_t)k * C + ch) * N;
  const T* sp = src + (int64_t)b * src_bs + pl;
  T* dp = dst + (int64_t)b * dst_bs + pl;
  const T* mp = mask ? mask + (int64_t)b * dst_bs + pl : nullptr;      // U: laid out as dU
  if (k == 0) mf_stb_body<T, 1>(L, sp, wb.w[0] + ch, dp, mp, H, W, ty0, tx0);
  else if (k == 1) mf_stb_body<T, 3>(L, sp, wb.w[1] + ch * 9, dp, mp, H, W, ty0, tx0);
  else if (k == 2) mf_stb_body<T, 5>(L, sp, wb.w[2] + ch * 25, dp, mp, H, W, ty0, tx0);
  else mf_stb_body<T, 7>(L, sp, wb.w[3] + ch * 49, dp, mp, H, W, ty0, tx0);
}

// ------------------------------------------------------------------ depthwise weight gradients
// grid (splits, C, B): dW[c][tap] = sum_p g[p] x[p + off(tap)] over the tiles split, split + splits, ...; partial row
// (b * splits + split) of [C][K*K].  MODE MF_RELU: x = relu(xin).
template <typename T, int K, int D, int MODE>
__global__ __launch_bounds__(256) void mefc_wgrad_kernel(const T* __restrict__ xin, int64_t x_bs, const T* __restrict__ g, int64_t g_bs,
                                                         float* __restrict__ part, int C, int H, int W, int tiles_x, int ntiles) {
  constexpr int R = (K / 2) * D, KK = K * K, LW = MfTile<R>::LW, H2 = K / 2;
  __shared__ float L[MfTile<R>::LT];
  __shared__ float red[4 * KK];
  const int split = blockIdx.x, splits = gridDim.x, ch = blockIdx.y, b = blockIdx.z;
  const int64_t N = (int64_t)H * W;
  const T* xp = xin + (int64_t)b * x_bs + ch * N;
  const T* gp = g + (int64_t)b * g_bs + ch * N;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float acc[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) acc[k] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * MF_TH, tx0 = (tile % tiles_x) * MF_TW;
    __syncthreads();
    mf_load<T, R, MODE>(L, xp, H, W, ty0, tx0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MF_RPT; ++j) {
      const int y = ty0 + ty + 8 * j, x = tx0 + tx;
      if (x < W && y < H) {
        const float gv = ld1(gp + (int64_t)y * W + x);
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
          for (int dx = 0; dx < K; ++dx)
            acc[dy * K + dx] = fmaf(gv, L[(ty + 8 * j + R + (dy - H2) * D) * LW + tx + R + (dx - H2) * D], acc[dy * K + dx]);
      }
    }
  }
  const float tot = mf_block_sum<KK>(acc, red);
  if ((int)threadIdx.x < KK) part[((int64_t)b * splits + split) * C * KK + (int64_t)ch * KK + threadIdx.x] = tot;
}

// ------------------------------------------------------------------ fold: M[b] = [w_i[b] out_w_i pw_i]_i
struct MfQ { const float* q[7]; };    // trailing 1x1s of ops 0..6 (sep pw2 k = 1..7, dil pw k = 3..7), [C][C]
struct MfGQ { float* q[7]; };
__device__ __forceinline__ const float* mf_pick(const MfQ& q, int i) {
  switch (i) {
    case 0: return q.q[0]; case 1: return q.q[1]; case 2: return q.q[2]; case 3: return q.q[3];
    case 4: return q.q[4]; case 5: return q.q[5]; default: return q.q[6];
  }
}
__device__ __forceinline__ float* mf_pick(const MfGQ& q, int i) {
  switch (i) {
    case 0: return q.q[0]; case 1: return q.q[1]; case 2: return q.q[2]; case 3: return q.q[3];
    case 4: return q.q[4]; case 5: return q.q[5]; default: return q.q[6];
  }
}
// A_i[o][c] = sum_k out_w[o][iC + k] pw_i[k][c] (i < 7), out_w[o][7C + c] (i = 7); fixed k order
__device__ __forceinline__ float mf_fold_a(const float* __restrict__ wout, const MfQ& q, int i, int o, int c, int C) {
  const int64_t C8 = 8 * (int64_t)C;
  if (i == 7) return wout[o * C8 + 7 * C + c];
  const float* qi = mf_pick(q, i);
  float a = 0.f;
  for (int k = 0; k < C; ++k) a = fmaf(wout[o * C8 + i * C + k], qi[(int64_t)k * C + c], a);
  return a;
}

// grid (8, C): panel i, row o.  wts [B][steps][8]; M [B][C][8C] fp32; Mb (same, bf16) and Mtb ([B][8C][C], bf16) or NULL.
__global__ __launch_bounds__(256) void mefc_fold_kernel(const float* __restrict__ wout, MfQ q, const float* __restrict__ wts, int steps,
                                                        int t, float* __restrict__ M, bf16* __restrict__ Mb, bf16* __restrict__ Mtb, int B,
                                                        int C) {
  const int i = blockIdx.x, o = blockIdx.y, c = threadIdx.x;
  if (c >= C) return;
  const int64_t C8 = 8 * (int64_t)C;
  const float a = mf_fold_a(wout, q, i, o, c, C);
  for (int b = 0; b < B; ++b) {
    const float v = wts[((int64_t)b * steps + t) * 8 + i] * a;
    const int64_t e = ((int64_t)b * C + o) * C8 + i * C + c;
    M[e] = v;
    if (Mb) {
      Mb[e] = (bf16)v;
      Mtb[((int64_t)b * C8 + i * C + c) * C + o] = (bf16)v;
    }
  }
}

// grid (8, C): panel i, row o.  G [B][C][8C] = dpre Z^T.  H_i[o][c] = sum_b w_i[b] G_i[b][o][c] -> Hs [8][C][C];
// d w_i[b] partial over row o: sum_c A_i[o][c] G_i[b][o][c] -> dwp [C][B][8]
__global__ __launch_bounds__(256) void mefc_fold_bwd_kernel(const float* __restrict__ G, const float* __restrict__ wout, MfQ q,
                                                            const float* __restrict__ wts, int steps, int t, float* __restrict__ Hs,
                                                            float* __restrict__ dwp, int B, int C) {
  __shared__ float red[4];
  const int i = blockIdx.x, o = blockIdx.y, c = threadIdx.x;
  const bool on = c < C;
  const int64_t C8 = 8 * (int64_t)C;
  const float a = on ? mf_fold_a(wout, q, i, o, c, C) : 0.f;
  float h = 0.f;
  for (int b = 0; b < B; ++b) {
    const float g = on ? G[((int64_t)b * C + o) * C8 + i * C + c] : 0.f;
    h = fmaf(wts[((int64_t)b * steps + t) * 8 + i], g, h);
    const float s = wave_sum(a * g);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dwp[((int64_t)o * B + b) * 8 + i] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
  }
  if (on) Hs[((int64_t)i * C + o) * C + c] = h;
}

// grid (8, C): panel i, row r.  d out_w[r][iC + c] = sum_k H_i[r][k] pw_i[c][k] (i = 7: H_7[r][c]);
// d pw_i[r][c] = sum_o out_w[o][iC + r] H_i[o][c].  acc: +=.
__global__ __launch_bounds__(256) void mefc_fold_wgrad_kernel(const float* __restrict__ Hs, const float* __restrict__ wout, MfQ q,
                                                              float* __restrict__ g_wout, MfGQ gq, int acc, int C) {
  const int i = blockIdx.x, r = blockIdx.y, c = threadIdx.x;
  if (c >= C) return;
  const int64_t C8 = 8 * (int64_t)C;
  const float* Hi = Hs + (int64_t)i * C * C;
  float v;
  if (i == 7) {
    v = Hi[(int64_t)r * C + c];
  } else {
    const float* qi = mf_pick(q, i);
    v = 0.f;
    for (int k = 0; k < C; ++k) v = fmaf(Hi[(int64_t)r * C + k], qi[(int64_t)c * C + k], v);
  }
  float* gw = g_wout + r * C8 + i * C + c;
  *gw = acc ? *gw + v : v;
  if (i < 7) {
    float d = 0.f;
    for (int o = 0; o < C; ++o) d = fmaf(wout[o * C8 + i * C + r], Hi[(int64_t)o * C + c], d);
    float* gp = mf_pick(gq, i) + (int64_t)r * C + c;
    *gp = acc ? *gp + d : d;
  }
}

// ------------------------------------------------------------------ routing head (OALayer, :227-247 + the softmax of :349)
// grid B.  pooled [B][C] (the global average pool); hpre [B][16 steps] (fc1 output, saved for the ReLU mask); wts [B][steps][8]
__global__ __launch_bounds__(256) void mefc_head_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ hpre,
                                                            float* __restrict__ wts, int C, int steps) {
  __shared__ float hs[16 * MF_MAX_STEPS], lg[8 * MF_MAX_STEPS];
  const int b = blockIdx.x, j = threadIdx.x, Hd = 16 * steps, Lo = 8 * steps;
  if (j < Hd) {
    float v = b1[j];
    for (int c = 0; c < C; ++c) v = fmaf(w1[(int64_t)j * C + c], pooled[(int64_t)b * C + c], v);
    hpre[(int64_t)b * Hd + j] = v;
    hs[j] = fmaxf(v, 0.f);
  }
  __syncthreads();
  if (j < Lo) {
    float v = b2[j];
    for (int k = 0; k < Hd; ++k) v = fmaf(w2[(int64_t)j * Hd + k], hs[k], v);
    lg[j] = v;
  }
  __syncthreads();
  if (j < steps) {
    float m = lg[j * 8];
    for (int i = 1; i < 8; ++i) m = fmaxf(m, lg[j * 8 + i]);
    float e[8], s = 0.f;
    for (int i = 0; i < 8; ++i) { e[i] = expf(lg[j * 8 + i] - m); s += e[i]; }
    for (int i = 0; i < 8; ++i) wts[((int64_t)b * steps + j) * 8 + i] = e[i] / s;
  }
}

// one workgroup, images in order.  dws [steps][B][8]: d w.  -> parameter gradients (acc: +=) and gp [B][C] = d pooled / N
// (the pool's gradient, a constant per (image, channel)).  scr: [B][8 steps] + [B][16 steps] floats.
__global__ __launch_bounds__(256) void mefc_head_bwd_kernel(const float* __restrict__ pooled, const float* __restrict__ hpre,
                                                            const float* __restrict__ wts, const float* __restrict__ dws,
                                                            const float* __restrict__ w1, const float* __restrict__ w2,
                                                            float* __restrict__ g_w1, float* __restrict__ g_b1, float* __restrict__ g_w2,
                                                            float* __restrict__ g_b2, float* __restrict__ gp, float* __restrict__ scr,
                                                            int acc, int B, int C, int steps, float inv_n) {
  const int Hd = 16 * steps, Lo = 8 * steps;
  float* dl = scr;
  float* dh = scr + (int64_t)B * Lo;
  for (int e = threadIdx.x; e < B * steps; e += 256) {          // softmax backward per (image, step)
    const int b = e / steps, t = e - b * steps;
    const float* w = wts + ((int64_t)b * steps + t) * 8;
    const float* d = dws + ((int64_t)t * B + b) * 8;
    float dot = 0.f;
    for (int i = 0; i < 8; ++i) dot = fmaf(w[i], d[i], dot);
    for (int i = 0; i < 8; ++i) dl[(int64_t)b * Lo + t * 8 + i] = w[i] * (d[i] - dot);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * Hd; e += 256) {
    const int b = e / Hd, j = e - b * Hd;
    float v = 0.f;
    for (int l = 0; l < Lo; ++l) v = fmaf(w2[(int64_t)l * Hd + j], dl[(int64_t)b * Lo + l], v);
    dh[e] = hpre[e] > 0.f ? v : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < Lo * Hd; e += 256) {
    const int l = e / Hd, j = e - l * Hd;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v = fmaf(dl[(int64_t)b * Lo + l], fmaxf(hpre[(int64_t)b * Hd + j], 0.f), v);
    g_w2[e] = acc ? g_w2[e] + v : v;
  }
  for (int l = threadIdx.x; l < Lo; l += 256) {
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += dl[(int64_t)b * Lo + l];
    g_b2[l] = acc ? g_b2[l] + v : v;
  }
  for (int e = threadIdx.x; e < Hd * C; e += 256) {
    const int j = e / C, c = e - j * C;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v = fmaf(dh[(int64_t)b * Hd + j], pooled[(int64_t)b * C + c], v);
    g_w1[e] = acc ? g_w1[e] + v : v;
  }
  for (int j = threadIdx.x; j < Hd; j += 256) {
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += dh[(int64_t)b * Hd + j];
    g_b1[j] = acc ? g_b1[j] + v : v;
  }
  for (int e = threadIdx.x; e < B * C; e += 256) {
    const int b = e / C, c = e - b * C;
    float v = 0.f;
    for (int j = 0; j < Hd; ++j) v = fmaf(w1[(int64_t)j * C + c], dh[(int64_t)b * Hd + j], v);
    gp[e] = v * inv_n;
  }
}

// ------------------------------------------------------------------ element-wise steps
enum { MF_EW_RES = 0, MF_EW_RES_BWD, MF_EW_MASK, MF_EW_RELU, MF_EW_ADDC };
// RES: o = relu(relu(a) + b) (a = pre, b = s);  RES_BWD: o = a (b > 0)(c > 0) (a = dout, b = out, c = pre);  MASK: o = a (b > 0);
// RELU: o = relu(a);  ADDC: o = a + cst[plane]  (plane = index / N).  o may be a (in place).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void mefc_ew_kernel(const T* a, const T* __restrict__ b, const T* __restrict__ c, T* o,
                                                      const float* __restrict__ cst, int64_t n, int64_t N) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float av = ld1(a + e);
    float v;
    if (MODE == MF_EW_RES) v = fmaxf(fmaxf(av, 0.f) + ld1(b + e), 0.f);
    else if (MODE == MF_EW_RES_BWD) v = (ld1(b + e) > 0.f && ld1(c + e) > 0.f) ? av : 0.f;
    else if (MODE == MF_EW_MASK) v = ld1(b + e) > 0.f ? av : 0.f;
    else if (MODE == MF_EW_RELU) v = fmaxf(av, 0.f);
    else v = av + cst[e / N];
    st1(o + e, v);
  }
}

template <typename T, int MODE>
static int mf_ew(const void* a, const void* b, const void* c, void* o, const float* cst, int64_t n, int64_t N, hipStream_t st) {
  ProfScope ps(st, K_MEFC_EW, 3.0 * n * sizeof(T), (double)n);
  hipLaunchKernelGGL((mefc_ew_kernel<T, MODE>), dim3(cdiv_cap(n, 256, 8192)), dim3(256), 0, st, (const T*)a, (const T*)b, (const T*)c, (T*)o, cst, n, N);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

template <typename T, int K, int D, int MODE>
static int mf_wgrad(const void* x, int64_t x_bs, const void* g, int64_t g_bs, float* part, float* out, int acc, int B, int C, int H,
                    int W, hipStream_t st) {
  const int splits = mf_splits(H, W);
  {
    const double n = (double)B * C * H * W;
    ProfScope ps(st, K_MEFC_WGRAD, 2.0 * n * sizeof(T), 2.0 * K * K * n);
    hipLaunchKernelGGL((mefc_wgrad_kernel<T, K, D, MODE>), dim3(splits, C, B), dim3(256), 0, st, (const T*)x, x_bs, (const T*)g, g_bs,
                       part, C, H, W, mf_tiles_x(W), mf_tiles(H, W));
    MI_LAUNCH_CHECK();
  }
  const int64_t cols = (int64_t)C * K * K;
  return launch_reduce_rows(part, out, (int64_t)B * splits, cols, cols, acc, 1.0f, st);
}

// ------------------------------------------------------------------ host side: layouts
// the per-image products: pre[b] = M[b] Z[b] (K = 8C) and dZ[b] = M[b]^T dpre[b] (K = C, 8C outputs); bf16 images of M / M^T
static mi_pw_desc mf_out_desc(const void* z, const float* M, const void* Mb, void* pre, int B, int C, int64_t N, int dt) {
  return per_image(conv1x1(z, 8 * C, M, false, 8 * C, nullptr, nullptr, pre, C, B, N, dt), Mb);
}
static mi_pw_desc mf_dz_desc(const void* dpre, const float* M, const void* Mtb, void* dz, int B, int C, int64_t N, int dt) {
  return per_image(conv1x1(dpre, C, M, true, 8 * C, nullptr, nullptr, dz, 8 * C, B, N, dt), Mtb);
}

struct MfStep { void* s; void* d1; void* u; void* z; void* pre; float* M; void* Mb; void* Mtb; };
struct MfSaved { float* pooled; float* hpre; float* wts; MfStep st[MF_MAX_STEPS]; void* s_alt; size_t bytes; };
// train: every step's planes (s_t, D1, U, Z, pre, M); inference: one set, reused by every step, and a second s plane
static MfSaved mf_saved_layout(const mi_mefc_shape* s, void* base, bool train) {
  const size_t B = s->B, C = s->C, N = (size_t)s->H * s->W;
  const int dt = s->dtype;
  Carver cv(base);
  MfSaved r;
  memset(&r, 0, sizeof(r));
  r.pooled = cv.take<float>(fbytes(B * C));
  r.hpre = cv.take<float>(fbytes(B * 16 * s->steps));
  r.wts = cv.take<float>(fbytes(B * 8 * s->steps));
  const int nst = train ? s->steps : 1;
  for (int t = 0; t < nst; ++t) {
    MfStep& q = r.st[t];
    q.s = cv.take(tbytes(B * C * N, dt));
    q.d1 = cv.take(tbytes(B * 4 * C * N, dt));
    q.u = cv.take(tbytes(B * 4 * C * N, dt));
    q.z = cv.take(tbytes(B * 8 * C * N, dt));
    q.pre = cv.take(tbytes(B * C * N, dt));
    q.M = cv.take<float>(fbytes(B * C * 8 * C));
    q.Mb = cv.take(tbytes(B * C * 8 * C, MI_BF16));
    q.Mtb = cv.take(tbytes(B * C * 8 * C, MI_BF16));
  }
  if (!train) {
    for (int t = 1; t < s->steps; ++t) r.st[t] = r.st[0];
    r.s_alt = cv.take(tbytes(B * C * N, dt));
  }
  r.bytes = cv.off;
  return r;
}

struct MfWs {
  void* pw_ws; void* gram_ws; float* part; float* G; float* Hs; float* dwp; float* dws; float* gp; float* hscr;
  MfSaved inf; void* dsa; void* dsb; void* dpre; void* dz; void* du; void* dd1; size_t bytes;
};
static MfWs mf_ws_layout(const mi_mefc_shape* s, void* base) {
  const int B = s->B, C = s->C, dt = s->dtype;
  const int64_t N = (int64_t)s->H * s->W;
  Carver cv(base);
  MfWs w;
  // preprocess and its transpose, pw1 and its transpose (slices of the 4C-plane tensors), the two per-image products
  w.pw_ws = cv.take(max_of({pw_ws_bytes(probe1x1(C, C, false, B, N, dt)), pw_ws_bytes(probe1x1(C, C, true, B, N, dt)),
                            pw_ws_bytes(probe1x1(C, C, false, B, N, dt, 4 * C * N, 4 * C * N)),
                            pw_ws_bytes(probe1x1(C, C, true, B, N, dt, 4 * C * N, 4 * C * N)),
                            pw_ws_bytes(per_image(probe1x1(8 * C, C, false, B, N, dt))),
                            pw_ws_bytes(per_image(probe1x1(C, 8 * C, true, B, N, dt)))}));
  // G[b] = dpre[b] Z[b]^T per image, the pw1 and the preprocess weight gradients
  w.gram_ws = cv.take(max_of({gram_ws_bytes(probe_wgrad(C, 8 * C, B, N, dt, 0)),
                              gram_ws_bytes(probe_wgrad(C, C, B, N, dt, 1, 4 * C * N, 4 * C * N)),
                              gram_ws_bytes(probe_wgrad(C, C, B, N, dt))}));
  w.part = cv.take<float>(fbytes((size_t)B * mf_splits(s->H, s->W) * C * 49));
  w.G = cv.take<float>(fbytes((size_t)B * C * 8 * C));
  w.Hs = cv.take<float>(fbytes((size_t)8 * C * C));
  w.dwp = cv.take<float>(fbytes((size_t)C * B * 8));
  w.dws = cv.take<float>(fbytes((size_t)s->steps * B * 8));
  w.gp = cv.take<float>(fbytes((size_t)B * C));
  w.hscr = cv.take<float>(fbytes((size_t)B * 24 * s->steps));
  const size_t mark = cv.off;
  w.inf = mf_saved_layout(s, base ? (char*)base + mark : nullptr, false);
  Carver big(base ? (char*)base + mark : nullptr);
  const size_t plane = tbytes((size_t)B * C * N, dt);
  w.dsa = big.take(plane);
  w.dsb = big.take(plane);
  w.dpre = big.take(plane);
  w.dz = big.take(tbytes((size_t)B * 8 * C * N, dt));
  w.du = big.take(tbytes((size_t)B * 4 * C * N, dt));
  w.dd1 = big.take(tbytes((size_t)B * 4 * C * N, dt));
  w.bytes = mark + max_of({w.inf.bytes, big.off});
  return w;
}

static int mf_check(const mi_mefc_shape* s) {
  MI_CHECK_ARG(s, "mefc: null shape");
  MI_CHECK_ARG(s->B > 0 && s->C > 0 && s->H > 0 && s->W > 0, "mefc: bad shape");
  MI_CHECK_ARG(s->C <= MF_MAX_C, "mefc: C=%d not covered (C <= %d)", s->C, MF_MAX_C);
  MI_CHECK_ARG(s->steps >= 1 && s->steps <= MF_MAX_STEPS, "mefc: steps=%d not covered (1 <= steps <= %d)", s->steps, MF_MAX_STEPS);
  MI_CHECK_ARG((int64_t)s->B * 8 * s->steps <= (1 << 20), "mefc: batch too large");
  MI_CHECK_ARG(s->B <= 65535, "mefc: B=%d too large", s->B);
  MI_CHECK_ARG(s->dtype == MI_F32 || s->dtype == MI_BF16, "mefc: bad dtype %d", s->dtype);
  return MI_OK;
}
static int mf_check_params(const mi_mefc_shape* s, const mi_mefc_params* p) {
  MI_CHECK_ARG(p && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && p->pre_w && p->step, "mefc: null parameter");
  for (int t = 0; t < s->steps; ++t) {
    const mi_mefc_step_params& q = p->step[t];
    for (int k = 0; k < 4; ++k)
      MI_CHECK_ARG(q.sep_dw1[k] && q.sep_pw1[k] && q.sep_dw2[k] && q.sep_pw2[k], "mefc: null SepConv weight (step %d)", t);
    for (int k = 0; k < 3; ++k) MI_CHECK_ARG(q.dil_dw[k] && q.dil_pw[k], "mefc: null DilConv weight (step %d)", t);
    MI_CHECK_ARG(q.out_w, "mefc: null out weight (step %d)", t);
  }
  return MI_OK;
}

static MfW7 mf_w7(const mi_mefc_step_params& q) {
  MfW7 a;
  for (int k = 0; k < 4; ++k) a.w[k] = q.sep_dw1[k];
  for (int k = 0; k < 3; ++k) a.w[4 + k] = q.dil_dw[k];
  return a;
}
static MfW4 mf_w4(const mi_mefc_step_params& q) {
  MfW4 a;
  for (int k = 0; k < 4; ++k) a.w[k] = q.sep_dw2[k];
  return a;
}
static MfQ mf_q(const mi_mefc_step_params& q) {
  MfQ a;
  for (int k = 0; k < 4; ++k) a.q[k] = q.sep_pw2[k];
  for (int k = 0; k < 3; ++k) a.q[4 + k] = q.dil_pw[k];
  return a;
}

template <typename T>
static void mf_launch_sta(const void* s, const MfW7& wa, void* d1, void* z, int B, int C, int H, int W, hipStream_t st) {
  hipLaunchKernelGGL((mefc_sta_fwd_kernel<T>), dim3(mf_tiles(H, W), C, B), dim3(256), 0, st, (const T*)s, wa, (T*)d1, (T*)z, C, H, W,
                     mf_tiles_x(W));
}
template <typename T>
static void mf_launch_stb(const void* src, int64_t src_bs, const MfW4& wb, void* dst, int64_t dst_bs, const void* mask, int B, int C,
                          int H, int W, hipStream_t st) {
  hipLaunchKernelGGL((mefc_stb_kernel<T>), dim3(mf_tiles(H, W), 4 * C, B), dim3(256), 0, st, (const T*)src, src_bs, wb, (T*)dst,
                     dst_bs, (const T*)mask, C, H, W, mf_tiles_x(W));
}
template <typename T>
static void mf_launch_sta_bwd(const void* dd1, const void* dz, const void* dout, const void* out, const MfW7& wa, void* ds, int B,
                              int C, int H, int W, hipStream_t st) {
  hipLaunchKernelGGL((mefc_sta_bwd_kernel<T>), dim3(mf_tiles(H, W), C, B), dim3(256), 0, st, (const T*)dd1, (const T*)dz,
                     (const T*)dout, (const T*)out, wa, (T*)ds, C, H, W, mf_tiles_x(W));
}

}  // namespace mi

using namespace mi;

extern "C" size_t mi_mefc_saved_bytes(const mi_mefc_shape* s) {
  if (mf_check(s) != MI_OK) return 0;
  return mf_saved_layout(s, nullptr, true).bytes;
}
extern "C" size_t mi_mefc_workspace(const mi_mefc_shape* s) {
  if (mf_check(s) != MI_OK) return 0;
  return mf_ws_layout(s, nullptr).bytes;
}

extern "C" int mi_mefc_fwd(const mi_mefc_shape* s, const mi_mefc_params* p, const void* x, void* out, void* saved, void* ws,
                           void* stream) {
  MI_TRY(mf_check(s));
  MI_TRY(mf_check_params(s, p));
  MI_CHECK_ARG(x && out && ws, "mefc_fwd: null pointer");
  return with_dtype(s->dtype, "mefc_fwd", [&](auto tag) -> int {
    using T = decltype(tag);
    hipStream_t st = (hipStream_t)stream;
    const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype, steps = s->steps;
    const int64_t N = (int64_t)H * W, CN = (int64_t)C * N;
    const bool train = saved != nullptr;
    MfWs w = mf_ws_layout(s, ws);
    MfSaved sv = train ? mf_saved_layout(s, saved, true) : w.inf;
    // routing weights (OALayer + softmax, :346-349)
    MI_TRY(mi_gap_fwd(x, sv.pooled, B, C, N, dt, stream));
    {
      ProfScope ps(st, K_MEFC_HEAD, 4.0 * (16.0 * steps * C + 128.0 * steps * steps) * B, 2.0 * (16.0 * steps * C + 128.0 * steps * steps) * B);
      hipLaunchKernelGGL(mefc_head_fwd_kernel, dim3(B), dim3(256), 0, st, sv.pooled, p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, sv.hpre,
                         sv.wts, C, steps);
      MI_LAUNCH_CHECK();
    }
    // s0 = relu(preprocess(x))  (:217 ReLUConv)
    void* cur = sv.st[0].s;
    mi_pw_desc d0 = conv1x1(x, C, p->pre_w, false, C, nullptr, nullptr, cur, C, B, N, dt);
    MI_TRY(mi_pw_gemm(&d0, w.pw_ws, stream));
    MI_TRY((mf_ew<T, MF_EW_RELU>(cur, nullptr, nullptr, cur, nullptr, B * CN, N, st)));
    for (int t = 0; t < steps; ++t) {
      const MfStep& q = sv.st[t];
      const mi_mefc_step_params& pp = p->step[t];
      void* nxt = t == steps - 1 ? out : (train ? sv.st[t + 1].s : (cur == sv.s_alt ? sv.st[0].s : sv.s_alt));
      {
        const double n = (double)B * CN;
        ProfScope ps(st, K_MEFC_STA, 8.0 * n * dtype_size(dt), 2.0 * (84 + 83 + 9) * n);
        mf_launch_sta<T>(cur, mf_w7(pp), q.d1, q.z, B, C, H, W, st);
        MI_LAUNCH_CHECK();
      }
      for (int k = 0; k < 4; ++k) {     // U_k = pw1_k D1_k
        const size_t off = (size_t)k * CN * dtype_size(dt);
        mi_pw_desc d = conv1x1((const char*)q.d1 + off, C, pp.sep_pw1[k], false, C, nullptr, nullptr, (char*)q.u + off, C, B, N, dt, 4 * CN, 4 * CN);
        MI_TRY(mi_pw_gemm(&d, w.pw_ws, stream));
      }
      {
        const double n = (double)B * 4 * CN;
        ProfScope ps(st, K_MEFC_STB, 2.0 * n * dtype_size(dt), 2.0 * 21 * n);
        mf_launch_stb<T>(q.u, 4 * CN, mf_w4(pp), q.z, 8 * CN, nullptr, B, C, H, W, st);
        MI_LAUNCH_CHECK();
      }
      {
        const bool b16 = dt == MI_BF16;
        ProfScope ps(st, K_MEFC_FOLD, 4.0 * 8 * C * C * (1.0 + B * (b16 ? 2.0 : 1.0)), 2.0 * 7 * C * C * C);
        hipLaunchKernelGGL(mefc_fold_kernel, dim3(8, C), dim3(256), 0, st, pp.out_w, mf_q(pp), sv.wts, steps, t, q.M,
                           b16 ? (bf16*)q.Mb : nullptr, b16 ? (bf16*)q.Mtb : nullptr, B, C);
        MI_LAUNCH_CHECK();
      }
      mi_pw_desc d = mf_out_desc(q.z, q.M, dt == MI_BF16 ? q.Mb : nullptr, q.pre, B, C, N, dt);
      MI_TRY(mi_pw_gemm(&d, w.pw_ws, stream));
      MI_TRY((mf_ew<T, MF_EW_RES>(q.pre, cur, nullptr, nxt, nullptr, B * CN, N, st)));   // s = relu(relu(_out(.)) + s)  (:222-223)
      cur = nxt;
    }
    return MI_OK;
  });
}

extern "C" int mi_mefc_bwd(const mi_mefc_shape* s, const mi_mefc_params* p, const void* x, const void* out, const void* dout, void* dx,
                           const mi_mefc_grads* g, const void* saved, void* ws, void* stream) {
  MI_TRY(mf_check(s));
  MI_TRY(mf_check_params(s, p));
  MI_CHECK_ARG(x && out && dout && dx && g && saved && ws, "mefc_bwd: null pointer");
  MI_CHECK_ARG(g->fc1_w && g->fc1_b && g->fc2_w && g->fc2_b && g->pre_w && g->step, "mefc_bwd: null gradient buffer");
  for (int t = 0; t < s->steps; ++t) {
    const mi_mefc_step_grads& q = g->step[t];
    for (int k = 0; k < 4; ++k)
      MI_CHECK_ARG(q.sep_dw1[k] && q.sep_pw1[k] && q.sep_dw2[k] && q.sep_pw2[k], "mefc_bwd: null SepConv gradient (step %d)", t);
    for (int k = 0; k < 3; ++k) MI_CHECK_ARG(q.dil_dw[k] && q.dil_pw[k], "mefc_bwd: null DilConv gradient (step %d)", t);
    MI_CHECK_ARG(q.out_w, "mefc_bwd: null out gradient (step %d)", t);
  }
  return with_dtype(s->dtype, "mefc_bwd", [&](auto tag) -> int {
    using T = decltype(tag);
    hipStream_t st = (hipStream_t)stream;
    const int B = s->B, C = s->C, H = s->H, W = s->W, dt = s->dtype, steps = s->steps, acc = g->accumulate;
    const int64_t N = (int64_t)H * W, CN = (int64_t)C * N;
    const size_t es = dtype_size(dt);
    MfWs w = mf_ws_layout(s, ws);
    MfSaved sv = mf_saved_layout(s, const_cast<void*>(saved), true);
    const void* dcur = dout;
    for (int t = steps - 1; t >= 0; --t) {
      const MfStep& q = sv.st[t];
      const mi_mefc_step_params& pp = p->step[t];
      const mi_mefc_step_grads& gg = g->step[t];
      const void* s_out = t == steps - 1 ? out : sv.st[t + 1].s;
      void* ds = dcur == w.dsa ? w.dsb : w.dsa;
      // dpre = dout (s' > 0)(pre > 0)
      MI_TRY((mf_ew<T, MF_EW_RES_BWD>(dcur, s_out, q.pre, w.dpre, nullptr, B * CN, N, st)));
      // fold backward: G[b] = dpre[b] Z[b]^T -> d w_i[b], d out_w, d pw_i
      mi_gram_desc gd = wgrad_gram(w.dpre, C, q.z, 8 * C, B, N, dt, w.G, 0, 0);
      MI_TRY(mi_gram(&gd, w.gram_ws, stream));
      const MfQ qq = mf_q(pp);
      {
        ProfScope ps(st, K_MEFC_FOLD_BWD, 4.0 * B * 8 * C * C + 4.0 * 16 * C * C, 2.0 * 8 * C * C * (C + 2.0 * B) + 2.0 * 14 * C * C * C);
        hipLaunchKernelGGL(mefc_fold_bwd_kernel, dim3(8, C), dim3(256), 0, st, w.G, pp.out_w, qq, sv.wts, steps, t, w.Hs, w.dwp, B, C);
        MI_LAUNCH_CHECK();
        MfGQ gq;
        for (int k = 0; k < 4; ++k) gq.q[k] = gg.sep_pw2[k];
        for (int k = 0; k < 3; ++k) gq.q[4 + k] = gg.dil_pw[k];
        hipLaunchKernelGGL(mefc_fold_wgrad_kernel, dim3(8, C), dim3(256), 0, st, w.Hs, pp.out_w, qq, gg.out_w, gq, acc, C);
        MI_LAUNCH_CHECK();
      }
      MI_TRY(launch_reduce_rows(w.dwp, w.dws + (int64_t)t * B * 8, C, (int64_t)B * 8, (int64_t)B * 8, 0, 1.0f, st));
      // dZ[b] = M[b]^T dpre[b]
      mi_pw_desc dzd = mf_dz_desc(w.dpre, q.M, dt == MI_BF16 ? q.Mtb : nullptr, w.dz, B, C, N, dt);
      MI_TRY(mi_pw_gemm(&dzd, w.pw_ws, stream));
      // stencil B backward: dU_k = (U_k > 0) dw2_k^T dZ_k, and the dw2 weight gradients (input relu(U_k))
      {
        const double n = (double)B * 4 * CN;
        ProfScope ps(st, K_MEFC_STB_BWD, 3.0 * n * es, 2.0 * 21 * n);
        mf_launch_stb<T>(w.dz, 8 * CN, mf_w4(pp), w.du, 4 * CN, q.u, B, C, H, W, st);
        MI_LAUNCH_CHECK();
      }
      // the dw2 weight gradients run before the data gradients: all of them through one partial-row region, in stream order
      MI_TRY((mf_wgrad<T, 1, 1, MF_RELU>(q.u, 4 * CN, w.dz, 8 * CN, w.part, gg.sep_dw2[0], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 3, 1, MF_RELU>((const char*)q.u + CN * es, 4 * CN, (const char*)w.dz + CN * es, 8 * CN, w.part, gg.sep_dw2[1], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 5, 1, MF_RELU>((const char*)q.u + 2 * CN * es, 4 * CN, (const char*)w.dz + 2 * CN * es, 8 * CN, w.part, gg.sep_dw2[2], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 7, 1, MF_RELU>((const char*)q.u + 3 * CN * es, 4 * CN, (const char*)w.dz + 3 * CN * es, 8 * CN, w.part, gg.sep_dw2[3], acc, B, C, H, W, st)));
      // pw1: dD1_k = pw1_k^T dU_k, d pw1_k = sum_b dU_k D1_k^T
      for (int k = 0; k < 4; ++k) {
        const size_t off = (size_t)k * CN * es;
        mi_pw_desc d = conv1x1((const char*)w.du + off, C, pp.sep_pw1[k], true, C, nullptr, nullptr, (char*)w.dd1 + off, C, B, N, dt, 4 * CN, 4 * CN);
        MI_TRY(mi_pw_gemm(&d, w.pw_ws, stream));
        mi_gram_desc gw = wgrad_gram((const char*)w.du + off, C, (const char*)q.d1 + off, C, B, N, dt, gg.sep_pw1[k], acc, 1, 4 * CN, 4 * CN);
        MI_TRY(mi_gram(&gw, w.gram_ws, stream));
      }
      // stencil A backward: ds, plus the residual's gradient
      {
        const double n = (double)B * CN;
        ProfScope ps(st, K_MEFC_STA_BWD, 11.0 * n * es, 2.0 * (84 + 83 + 9) * n);
        mf_launch_sta_bwd<T>(w.dd1, w.dz, dcur, s_out, mf_w7(pp), ds, B, C, H, W, st);
        MI_LAUNCH_CHECK();
      }
      const char* d1 = (const char*)w.dd1;
      const char* dz = (const char*)w.dz;
      MI_TRY((mf_wgrad<T, 1, 1, MF_PLAIN>(q.s, CN, d1, 4 * CN, w.part, gg.sep_dw1[0], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 3, 1, MF_PLAIN>(q.s, CN, d1 + CN * es, 4 * CN, w.part, gg.sep_dw1[1], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 5, 1, MF_PLAIN>(q.s, CN, d1 + 2 * CN * es, 4 * CN, w.part, gg.sep_dw1[2], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 7, 1, MF_PLAIN>(q.s, CN, d1 + 3 * CN * es, 4 * CN, w.part, gg.sep_dw1[3], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 3, 2, MF_PLAIN>(q.s, CN, dz + 4 * CN * es, 8 * CN, w.part, gg.dil_dw[0], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 5, 2, MF_PLAIN>(q.s, CN, dz + 5 * CN * es, 8 * CN, w.part, gg.dil_dw[1], acc, B, C, H, W, st)));
      MI_TRY((mf_wgrad<T, 7, 2, MF_PLAIN>(q.s, CN, dz + 6 * CN * es, 8 * CN, w.part, gg.dil_dw[2], acc, B, C, H, W, st)));
      dcur = ds;
    }
    // through the preprocess ReLU and 1x1
    void* dpre0 = w.dpre;
    MI_TRY((mf_ew<T, MF_EW_MASK>(dcur, sv.st[0].s, nullptr, dpre0, nullptr, B * CN, N, st)));
    MI_TRY(conv1x1_bwd_input(dpre0, C, x, C, p->pre_w, g->pre_w, nullptr, dx, B, N, dt, acc, w.gram_ws, nullptr, w.pw_ws, st, false));
    // routing head: the d w of every step through the softmax and the MLP; the pooled gradient joins dx
    {
      ProfScope ps(st, K_MEFC_HEAD_BWD, 8.0 * (16.0 * steps * C + 128.0 * steps * steps) * B, 6.0 * (16.0 * steps * C + 128.0 * steps * steps) * B);
      hipLaunchKernelGGL(mefc_head_bwd_kernel, dim3(1), dim3(256), 0, st, sv.pooled, sv.hpre, sv.wts, w.dws, p->fc1_w, p->fc2_w, g->fc1_w,
                         g->fc1_b, g->fc2_w, g->fc2_b, w.gp, w.hscr, acc, B, C, steps, 1.0f / (float)N);
      MI_LAUNCH_CHECK();
    }
    return mf_ew<T, MF_EW_ADDC>(dx, nullptr, nullptr, dx, w.gp, B * CN, N, st);
  });
}
