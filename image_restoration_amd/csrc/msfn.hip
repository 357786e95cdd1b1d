// The stencils of DRSformer's mixed-scale FFN (MSFN, DRSformer_arch.py:62-98), between its two 1x1 projections:
//   stage 1: a = relu(dw3(h0)), b = relu(dw5(h0))                      depthwise 3x3 and 5x5 on the same 2h planes, one read of h0
//   stage 2: y[j] = relu(gdw3(x1)[j]), y[h + j] = relu(gdw5(x2)[j])    grouped, two input channels per group (2j, 2j + 1)
//            x1 = cat(a[:h], b[:h]), x2 = cat(a[h:], b[h:])            never materialised: channel k of x_br is a[br h + k] for
//                                                                      k < h, else b[br h + k - h] (for odd h one group reads
//                                                                      the last channel of a and the first of b)
// Tiles of 32 x 8 output pixels, one per thread, with a 2-pixel halo staged in LDS (zero outside the plane: the convs' padding).
// Backward: data gradients through the ReLU masks (a > 0, b > 0, y > 0), and weight / bias gradients as per-workgroup partial rows
// (fixed-order block sums, no atomics) summed over rows by launch_reduce_rows in a fixed order: bitwise reproducible.
#include "internal.h"

namespace mi {

constexpr int MS_TW = 32, MS_TH = 8, MS_R = 2, MS_LW = MS_TW + 2 * MS_R, MS_LH = MS_TH + 2 * MS_R, MS_LT = MS_LW * MS_LH;
constexpr int MS_MAX_SPLITS = 16;   // workgroups per (image, channel) in backward: each walks every splits-th tile

static inline int ms_tiles_x(int W) { return cdiv(W, MS_TW); }
static inline int ms_tiles(int H, int W) { return ms_tiles_x(W) * cdiv(H, MS_TH); }
int msfn_splits(int H, int W) {
  const int n = ms_tiles(H, W);
  return n < MS_MAX_SPLITS ? n : MS_MAX_SPLITS;
}

// plane tile (rows ty0 - 2 .. ty0 + 9, columns tx0 - 2 .. tx0 + 33) -> L; zero outside the plane.  mask (optional): times (mask > 0)
template <typename T>
__device__ __forceinline__ void ms_load(float* L, const T* __restrict__ p, const T* __restrict__ mask, int H, int W, int ty0, int tx0) {
  for (int e = threadIdx.x; e < MS_LT; e += 256) {
    const int ly = e / MS_LW, lx = e - ly * MS_LW;
    const int y = ty0 - MS_R + ly, x = tx0 - MS_R + lx;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t o = (int64_t)y * W + x;
      v = ld1(p + o);
      if (mask && !(ld1(mask + o) > 0.f)) v = 0.f;
    }
    L[e] = v;
  }
}

// Channel k (0 .. 2h-1) of x_br (br 0: x1, br 1: x2) of image b.
template <typename T>
__device__ __forceinline__ int64_t ms_src(int br, int k, int hd, int b, int64_t N, bool& from_b) {
  const int64_t C2 = 2 * (int64_t)hd;
  from_b = k >= hd;
  return ((int64_t)b * C2 + br * hd + (from_b ? k - hd : k)) * N;
}

// ------------------------------------------------------------------ stage 1
template <typename T>
__global__ __launch_bounds__(256) void msfn_s1_fwd_kernel(const T* __restrict__ h0, const float* __restrict__ w3,
                                                          const float* __restrict__ b3, const float* __restrict__ w5,
                                                          const float* __restrict__ b5, T* __restrict__ ao, T* __restrict__ bo,
                                                          int C2, int H, int W, int tiles_x) {
  __shared__ float L[MS_LT];
  const int ch = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * MS_TH, tx0 = (blockIdx.x % tiles_x) * MS_TW;
  const int64_t N = (int64_t)H * W, po = ((int64_t)b * C2 + ch) * N;
  ms_load<T>(L, h0 + po, nullptr, H, W, ty0, tx0);
  __syncthreads();
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, x = tx0 + tx, y = ty0 + ty;
  if (x >= W || y >= H) return;
  float s3 = b3 ? b3[ch] : 0.f, s5 = b5 ? b5[ch] : 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) s3 = fmaf(w3[ch * 9 + dy * 3 + dx], L[(ty + 1 + dy) * MS_LW + tx + 1 + dx], s3);
#pragma unroll
  for (int dy = 0; dy < 5; ++dy)
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) s5 = fmaf(w5[ch * 25 + dy * 5 + dx], L[(ty + dy) * MS_LW + tx + dx], s5);
  const int64_t o = po + (int64_t)y * W + x;
  st1(ao + o, fmaxf(s3, 0.f));
  st1(bo + o, fmaxf(s5, 0.f));
}

// grid (splits, 2h, B).  dza / dzb: gradients at the pre-activations of a / b.  dh0 = dw3^T dza + dw5^T dzb; partial rows of
// dw3 [2h][9], dw5 [2h][25], db3, db5 (row = b * splits + split).
template <typename T>
__global__ __launch_bounds__(256) void msfn_s1_bwd_kernel(const T* __restrict__ dza, const T* __restrict__ dzb, const T* __restrict__ h0,
                                                          const float* __restrict__ w3, const float* __restrict__ w5, T* __restrict__ dh0,
                                                          float* __restrict__ p3, float* __restrict__ p5, float* __restrict__ pb3,
                                                          float* __restrict__ pb5, int C2, int H, int W, int tiles_x, int ntiles) {
  __shared__ float L[3 * MS_LT];
  __shared__ float red[4 * 36];
  const int split = blockIdx.x, splits = gridDim.x, ch = blockIdx.y, b = blockIdx.z;
  const int64_t N = (int64_t)H * W, po = ((int64_t)b * C2 + ch) * N;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float wa[9], wb[25], acc[36];
#pragma unroll
  for (int k = 0; k < 9; ++k) wa[k] = w3[ch * 9 + k];
#pragma unroll
  for (int k = 0; k < 25; ++k) wb[k] = w5[ch * 25 + k];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * MS_TH, tx0 = (tile % tiles_x) * MS_TW;
    __syncthreads();
    ms_load<T>(L, dza + po, nullptr, H, W, ty0, tx0);
    ms_load<T>(L + MS_LT, dzb + po, nullptr, H, W, ty0, tx0);
    ms_load<T>(L + 2 * MS_LT, h0 + po, nullptr, H, W, ty0, tx0);
    __syncthreads();
    const int x = tx0 + tx, y = ty0 + ty;
    if (x < W && y < H) {
      const float* La = L;
      const float* Lb = L + MS_LT;
      const float* Lx = L + 2 * MS_LT;
      const float d3 = La[(ty + MS_R) * MS_LW + tx + MS_R], d5 = Lb[(ty + MS_R) * MS_LW + tx + MS_R];
      float dh = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          dh = fmaf(wa[dy * 3 + dx], La[(ty + 3 - dy) * MS_LW + tx + 3 - dx], dh);
          acc[dy * 3 + dx] = fmaf(d3, Lx[(ty + 1 + dy) * MS_LW + tx + 1 + dx], acc[dy * 3 + dx]);
        }
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          dh = fmaf(wb[dy * 5 + dx], Lb[(ty + 4 - dy) * MS_LW + tx + 4 - dx], dh);
          acc[9 + dy * 5 + dx] = fmaf(d5, Lx[(ty + dy) * MS_LW + tx + dx], acc[9 + dy * 5 + dx]);
        }
      acc[34] += d3;
      acc[35] += d5;
      st1(dh0 + po + (int64_t)y * W + x, dh);
    }
  }
  const float tot = block_sum4<36>(acc, red);
  const int n = threadIdx.x;
  const int64_t row = (int64_t)b * splits + split;
  if (n < 9) p3[row * C2 * 9 + ch * 9 + n] = tot;
  else if (n < 34) p5[row * C2 * 25 + ch * 25 + n - 9] = tot;
  else if (n == 34) pb3[row * C2 + ch] = tot;
  else if (n == 35) pb5[row * C2 + ch] = tot;
}

// ------------------------------------------------------------------ stage 2
template <typename T, int KS>
__device__ __forceinline__ void ms_s2_fwd_body(const float* L, const float* __restrict__ w, float bias, T* __restrict__ out, int H,
                                               int W, int ty0, int tx0) {
  constexpr int K2 = KS * KS, OF = MS_R - KS / 2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, x = tx0 + tx, y = ty0 + ty;
  if (x >= W || y >= H) return;
  float s = bias;
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) s = fmaf(w[e * K2 + dy * KS + dx], L[e * MS_LT + (ty + OF + dy) * MS_LW + tx + OF + dx], s);
  st1(out + (int64_t)y * W + x, fmaxf(s, 0.f));
}

// grid (tiles, 2h, B): output channel o = br h + j (br 0: gdw3 on x1, br 1: gdw5 on x2)
template <typename T>
__global__ __launch_bounds__(256) void msfn_s2_fwd_kernel(const T* __restrict__ a, const T* __restrict__ bsrc, const float* __restrict__ g3w,
                                                          const float* __restrict__ g3b, const float* __restrict__ g5w,
                                                          const float* __restrict__ g5b, T* __restrict__ y, int hd, int H, int W,
                                                          int tiles_x) {
  __shared__ float L[2 * MS_LT];
  const int o = blockIdx.y, b = blockIdx.z, br = o >= hd ? 1 : 0, j = o - br * hd;
  const int ty0 = (blockIdx.x / tiles_x) * MS_TH, tx0 = (blockIdx.x % tiles_x) * MS_TW;
  const int64_t N = (int64_t)H * W;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    bool fb;
    const int64_t so = ms_src<T>(br, 2 * j + e, hd, b, N, fb);
    ms_load<T>(L + e * MS_LT, (fb ? bsrc : a) + so, nullptr, H, W, ty0, tx0);
  }
  __syncthreads();
  T* out = y + ((int64_t)b * 2 * hd + o) * N;
  if (br == 0) ms_s2_fwd_body<T, 3>(L, g3w + j * 18, g3b ? g3b[j] : 0.f, out, H, W, ty0, tx0);
  else ms_s2_fwd_body<T, 5>(L, g5w + j * 50, g5b ? g5b[j] : 0.f, out, H, W, ty0, tx0);
}

// one output channel o = br h + j over the tiles of this workgroup: dz = dY (y > 0); the gradients of its two input channels,
// times their ReLU masks (x > 0: x is a or b), go to dza / dzb; partial row of dW [2][KS*KS] and db
template <typename T, int KS>
__device__ __forceinline__ void ms_s2_bwd_body(float* L, float* red, const T* __restrict__ dY, const T* __restrict__ yv,
                                               const T* __restrict__ x0, const T* __restrict__ x1, T* __restrict__ dx0,
                                               T* __restrict__ dx1, const float* __restrict__ w, float* __restrict__ pw,
                                               float* __restrict__ pb, int H, int W, int tiles_x, int ntiles, int split, int splits) {
  constexpr int K2 = KS * KS, RK = KS / 2, OF = MS_R - RK, NV = 2 * K2 + 1;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float wr[2 * K2], acc[NV];
#pragma unroll
  for (int k = 0; k < 2 * K2; ++k) wr[k] = w[k];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * MS_TH, tx0 = (tile % tiles_x) * MS_TW;
    __syncthreads();
    ms_load<T>(L, dY, yv, H, W, ty0, tx0);
    ms_load<T>(L + MS_LT, x0, nullptr, H, W, ty0, tx0);
    ms_load<T>(L + 2 * MS_LT, x1, nullptr, H, W, ty0, tx0);
    __syncthreads();
    const int x = tx0 + tx, y = ty0 + ty;
    if (x < W && y < H) {
      const float dz = L[(ty + MS_R) * MS_LW + tx + MS_R];
      acc[2 * K2] += dz;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float* Lx = L + (1 + e) * MS_LT;
        float d = 0.f;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy)
#pragma unroll
          for (int dx = 0; dx < KS; ++dx) {
            acc[e * K2 + dy * KS + dx] = fmaf(dz, Lx[(ty + OF + dy) * MS_LW + tx + OF + dx], acc[e * K2 + dy * KS + dx]);
            d = fmaf(wr[e * K2 + dy * KS + dx], L[(ty + MS_R + RK - dy) * MS_LW + tx + MS_R + RK - dx], d);
          }
        const float xv = Lx[(ty + MS_R) * MS_LW + tx + MS_R];
        st1((e ? dx1 : dx0) + (int64_t)y * W + x, xv > 0.f ? d : 0.f);
      }
    }
  }
  const float tot = block_sum4<NV>(acc, red);
  const int n = threadIdx.x;
  if (n < 2 * K2) pw[n] = tot;
  else if (n == 2 * K2) pb[0] = tot;
}

// grid (splits, 2h, B).  Partial rows (row = b * splits + split): dW of gdw3 [h][18], of gdw5 [h][50], db3 [h], db5 [h].
template <typename T>
__global__ __launch_bounds__(256) void msfn_s2_bwd_kernel(const T* __restrict__ dY, const T* __restrict__ yv, const T* __restrict__ a,
                                                          const T* __restrict__ bsrc, const float* __restrict__ g3w,
                                                          const float* __restrict__ g5w, T* __restrict__ dza, T* __restrict__ dzb,
                                                          float* __restrict__ p3, float* __restrict__ p5, float* __restrict__ pb3,
                                                          float* __restrict__ pb5, int hd, int H, int W, int tiles_x, int ntiles) {
  __shared__ float L[3 * MS_LT];
  __shared__ float red[4 * 51];
  const int split = blockIdx.x, splits = gridDim.x, o = blockIdx.y, b = blockIdx.z, br = o >= hd ? 1 : 0, j = o - br * hd;
  const int64_t N = (int64_t)H * W, yo = ((int64_t)b * 2 * hd + o) * N, row = (int64_t)b * splits + split;
  bool f0, f1;
  const int64_t s0 = ms_src<T>(br, 2 * j, hd, b, N, f0), s1 = ms_src<T>(br, 2 * j + 1, hd, b, N, f1);
  const T* x0 = (f0 ? bsrc : a) + s0;
  const T* x1 = (f1 ? bsrc : a) + s1;
  T* d0 = (f0 ? dzb : dza) + s0;
  T* d1 = (f1 ? dzb : dza) + s1;
  if (br == 0)
    ms_s2_bwd_body<T, 3>(L, red, dY + yo, yv + yo, x0, x1, d0, d1, g3w + j * 18, p3 + row * hd * 18 + j * 18, pb3 + row * hd + j, H,
                         W, tiles_x, ntiles, split, splits);
  else
    ms_s2_bwd_body<T, 5>(L, red, dY + yo, yv + yo, x0, x1, d0, d1, g5w + j * 50, p5 + row * hd * 50 + j * 50, pb5 + row * hd + j, H,
                         W, tiles_x, ntiles, split, splits);
}

// ------------------------------------------------------------------ launchers
// partial-row floats of one backward stage (both stages take the same: 2h (9 + 25 + 2) == h (18 + 50 + 2) + 2h)
size_t msfn_part_floats(int B, int hd, int H, int W) { return (size_t)B * msfn_splits(H, W) * 2 * hd * 36; }

int launch_msfn_s1_fwd(const void* h0, const float* w3, const float* b3, const float* w5, const float* b5, void* a, void* b, int B,
                       int hd, int H, int W, int dtype, hipStream_t st) {
  MI_CHECK_ARG(h0 && w3 && w5 && a && b, "msfn: null pointer in stage 1");
  const int C2 = 2 * hd, tx = ms_tiles_x(W);
  const double n = (double)B * C2 * H * W;
  ProfScope ps(st, K_MSFN_S1, 3.0 * n * dtype_size(dtype), 2.0 * 34 * n);
  dim3 grid(ms_tiles(H, W), C2, B);
  return with_dtype(dtype, "msfn_s1_fwd", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((msfn_s1_fwd_kernel<T>), grid, dim3(256), 0, st, (const T*)h0, w3, b3, w5, b5, (T*)a, (T*)b, C2, H, W, tx);
  });
}

int launch_msfn_s2_fwd(const void* a, const void* b, const float* g3w, const float* g3b, const float* g5w, const float* g5b, void* y,
                       int B, int hd, int H, int W, int dtype, hipStream_t st) {
  MI_CHECK_ARG(a && b && g3w && g5w && y, "msfn: null pointer in stage 2");
  const int tx = ms_tiles_x(W);
  const double n = (double)B * hd * H * W;
  ProfScope ps(st, K_MSFN_S2, 6.0 * n * dtype_size(dtype), 2.0 * 2 * (9 + 25) * n);
  dim3 grid(ms_tiles(H, W), 2 * hd, B);
  return with_dtype(dtype, "msfn_s2_fwd", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((msfn_s2_fwd_kernel<T>), grid, dim3(256), 0, st, (const T*)a, (const T*)b, g3w, g3b, g5w, g5b, (T*)y, hd, H, W, tx);
  });
}

// dY: gradient of cat(y1, y2) [B][2h]; y: its forward value; a, b: stage-1 outputs.  -> dza, dzb (gradients at the stage-1
// pre-activations) and the gradients of gdw3 / gdw5 (weights [h][2][k][k], biases [h] or NULL).
int launch_msfn_s2_bwd(const void* dY, const void* y, const void* a, const void* b, const float* g3w, const float* g5w, void* dza,
                       void* dzb, float* g_g3w, float* g_g3b, float* g_g5w, float* g_g5b, int accumulate, float* part, int B, int hd,
                       int H, int W, int dtype, hipStream_t st) {
  MI_CHECK_ARG(dY && y && a && b && g3w && g5w && dza && dzb && g_g3w && g_g5w && part, "msfn: null pointer in stage-2 backward");
  const int splits = msfn_splits(H, W), tx = ms_tiles_x(W), nt = ms_tiles(H, W);
  const int64_t rows = (int64_t)B * splits;
  float* p3 = part;
  float* p5 = p3 + rows * hd * 18;
  float* pb3 = p5 + rows * hd * 50;
  float* pb5 = pb3 + rows * hd;
  dim3 grid(splits, 2 * hd, B);
  MI_TRY(with_dtype(dtype, "msfn_s2_bwd", [&](auto tag) {
    using T = decltype(tag);
    const double n = (double)B * hd * H * W;
    ProfScope ps(st, K_MSFN_S2_BWD, 10.0 * n * sizeof(T), 4.0 * 2 * (9 + 25) * n);
    hipLaunchKernelGGL((msfn_s2_bwd_kernel<T>), grid, dim3(256), 0, st, (const T*)dY, (const T*)y, (const T*)a, (const T*)b, g3w, g5w,
                       (T*)dza, (T*)dzb, p3, p5, pb3, pb5, hd, H, W, tx, nt);
  }));
  MI_TRY(launch_reduce_rows(p3, g_g3w, rows, (int64_t)hd * 18, (int64_t)hd * 18, accumulate, 1.0f, st));
  MI_TRY(launch_reduce_rows(p5, g_g5w, rows, (int64_t)hd * 50, (int64_t)hd * 50, accumulate, 1.0f, st));
  if (g_g3b) MI_TRY(launch_reduce_rows(pb3, g_g3b, rows, hd, hd, accumulate, 1.0f, st));
  if (g_g5b) MI_TRY(launch_reduce_rows(pb5, g_g5b, rows, hd, hd, accumulate, 1.0f, st));
  return MI_OK;
}

int launch_msfn_s1_bwd(const void* dza, const void* dzb, const void* h0, const float* w3, const float* w5, void* dh0, float* g_w3,
                       float* g_b3, float* g_w5, float* g_b5, int accumulate, float* part, int B, int hd, int H, int W, int dtype,
                       hipStream_t st) {
  MI_CHECK_ARG(dza && dzb && h0 && w3 && w5 && dh0 && g_w3 && g_w5 && part, "msfn: null pointer in stage-1 backward");
  const int C2 = 2 * hd, splits = msfn_splits(H, W), tx = ms_tiles_x(W), nt = ms_tiles(H, W);
  const int64_t rows = (int64_t)B * splits;
  float* p3 = part;
  float* p5 = p3 + rows * C2 * 9;
  float* pb3 = p5 + rows * C2 * 25;
  float* pb5 = pb3 + rows * C2;
  dim3 grid(splits, C2, B);
  MI_TRY(with_dtype(dtype, "msfn_s1_bwd", [&](auto tag) {
    using T = decltype(tag);
    const double n = (double)B * C2 * H * W;
    ProfScope ps(st, K_MSFN_S1_BWD, 4.0 * n * sizeof(T), 4.0 * 34 * n);
    hipLaunchKernelGGL((msfn_s1_bwd_kernel<T>), grid, dim3(256), 0, st, (const T*)dza, (const T*)dzb, (const T*)h0, w3, w5, (T*)dh0, p3, p5,
                       pb3, pb5, C2, H, W, tx, nt);
  }));
  MI_TRY(launch_reduce_rows(p3, g_w3, rows, (int64_t)C2 * 9, (int64_t)C2 * 9, accumulate, 1.0f, st));
  MI_TRY(launch_reduce_rows(p5, g_w5, rows, (int64_t)C2 * 25, (int64_t)C2 * 25, accumulate, 1.0f, st));
  if (g_b3) MI_TRY(launch_reduce_rows(pb3, g_b3, rows, C2, C2, accumulate, 1.0f, st));
  if (g_b5) MI_TRY(launch_reduce_rows(pb5, g_b5, rows, C2, C2, accumulate, 1.0f, st));
  return MI_OK;
}

}  // namespace mi
