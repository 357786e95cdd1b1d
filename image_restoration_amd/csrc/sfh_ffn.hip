// SFHformer's FFN (SFHformer.py:76-119) and TokenMixer_For_Local (:122-140): one "segmented depthwise" kernel family and the two
// module launch sequences on top of it.  The channel axis of [B, S s, H, W] is cut into S segments of s channels; segment k has
// its own depthwise stencil (ks_k, dil_k), zero padding dil (ks - 1) / 2, or none (ks == 1: identity):
//   FFN    (1,1) (3,1) (5,1) (7,1) over the four dim/2-wide segments of h = conv_init(x), then g = gelu_erf(u)
//   local  (3,1) (3,2) over the two dim/2-wide halves of x, no activation
// Exactly these two tap lists are instantiated.  One workgroup of 256 threads per (tile, channel, image); a tile is 64 x 16
// output pixels, four consecutive pixels of a row per thread, so that the staging loads, the window reads from LDS and the
// stores are all 4 wide.  The tile and its halo (up to 3) are staged in LDS as fp32 in 72-float rows: 4 columns of left margin
// (plane column tx0 - 4 sits at LDS column 0), so that every 4-pixel chunk of the plane is a 16-byte chunk of the LDS row; zeros
// outside the plane (the convs' padding).  Rows are loaded 4 wide where W % 4 == 0 and the tensors are 16-byte aligned (then a
// chunk is wholly inside or wholly outside the plane); otherwise element by element with bounds.  Identity channels use no LDS.
// Backward: du = dg gelu_erf'(u) is formed while dg is staged (no elementwise pass), g = gelu_erf(u) is written again for the
// tile's interior (conv_fina's weight gradient reads it), dh = stencil^T(du); weight and bias gradients as per-workgroup partial
// rows (fixed-order block sums, no atomics) summed over rows by launch_reduce_rows in a fixed order: bitwise reproducible.
// In bf16 the forward takes g from u AS STORED (rounded), so that the backward's g and gelu' are those of the forward.
#include "internal.h"

namespace mi {
namespace {

constexpr int SF_TW = 64, SF_TH = 16, SF_PAD = 4, SF_LW = SF_TW + 2 * SF_PAD, SF_CHUNKS = SF_LW / 4, SF_MAXR = 3;
constexpr int SF_MAXLT = (SF_TH + 2 * SF_MAXR) * SF_LW;   // floats of the largest staged tile (22 x 72)
constexpr int SF_THREADS = 256, SF_MAX_SPLITS = 16;       // backward: workgroups per plane, each walks every splits-th tile
constexpr int SF_MAX_DIM = 256, SF_MAX_SEG = 4;
enum { SF_FFN = 0, SF_LOCAL = 1 };

struct SegPtrs { const float* w[SF_MAX_SEG]; const float* b[SF_MAX_SEG]; };
struct SegParts { float* p[SF_MAX_SEG]; };   // partial rows of segment k: [rows][s (ks^2 + 1)], the s ks^2 weight columns first

// Phi(x) and phi(x) of the erf-form GELU.  bf16 activations: gelu_parts (common.h), whose Abramowitz-Stegun erf is exact to 1.5e-7,
// far under a bf16 step.  fp32 activations: libm's erfc and exp.  The bias and weight gradients of the stencils are sums of
// dg gelu'(u) over a plane that cancel to ~1 / sqrt(pixels) of their terms, and an error of 1.5e-7 per term, which does not average
// out the way rounding does, came to 4.1 x the fp32 host error of such a sum (measured: conv1_1's bias gradient on a 40 x 70 plane).
template <typename T> __device__ __forceinline__ void sf_gelu_parts(float x, float& cdf, float& pdf) { gelu_parts(x, cdf, pdf); }
template <> __device__ __forceinline__ void sf_gelu_parts<float>(float x, float& cdf, float& pdf) {
  cdf = 0.5f * erfcf(-0.70710678118654752440f * x);
  pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
}
template <typename T> __device__ __forceinline__ float sf_gelu(float x) {
  float cdf, pdf;
  sf_gelu_parts<T>(x, cdf, pdf);
  return x * cdf;
}

// plane rows ty0 - R .. ty0 + 15 + R, columns tx0 - 4 .. tx0 + 67 -> L (zero outside the plane).  GELU: p is dg, the value staged
// is dg gelu_erf'(u), and gelu_erf(u) goes to gp for the tile's interior.
template <typename T, int R, bool GELU>
__device__ __forceinline__ void sf_stage(float* L, const T* __restrict__ p, const T* __restrict__ up, T* __restrict__ gp, int H, int W,
                                         int ty0, int tx0, bool vec) {
  constexpr int LH = SF_TH + 2 * R;
  for (int e = threadIdx.x; e < LH * SF_CHUNKS; e += SF_THREADS) {
    const int ly = e / SF_CHUNKS, c = e - ly * SF_CHUNKS;
    const int y = ty0 - R + ly, x0 = tx0 - SF_PAD + 4 * c;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < H && x0 >= 0 && x0 < W) {
      const int64_t o = (int64_t)y * W + x0;
      [[maybe_unused]] const bool inner = GELU && c >= 1 && c <= SF_TW / 4 && ly >= R && ly < R + SF_TH;
      if (vec) {
        Vec<T, 4>::ld(p + o, v);
        if constexpr (GELU) {
          float uu[4], g[4];
          Vec<T, 4>::ld(up + o, uu);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float cdf, pdf;
            sf_gelu_parts<T>(uu[i], cdf, pdf);
            g[i] = uu[i] * cdf;
            v[i] *= cdf + uu[i] * pdf;
          }
          if (inner) Vec<T, 4>::st(gp + o, g);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (x0 + i >= W) break;
          v[i] = ld1(p + o + i);
          if constexpr (GELU) {
            const float uu = ld1(up + o + i);
            float cdf, pdf;
            sf_gelu_parts<T>(uu, cdf, pdf);
            v[i] *= cdf + uu * pdf;
            if (inner) st1(gp + o + i, uu * cdf);
          }
        }
      }
    }
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(L + ly * SF_LW + 4 * c) = t;
  }
}

// the 12 floats of LDS row `row` from column 4 t: plane columns x - 4 .. x + 7 for this thread's first pixel x
__device__ __forceinline__ void sf_window(const float* row, float* win) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(row + 4 * q);
    win[4 * q] = t[0]; win[4 * q + 1] = t[1]; win[4 * q + 2] = t[2]; win[4 * q + 3] = t[3];
  }
}

// four pixels of one row to a plane: 4 wide where the row allows it, else element by element up to the plane's edge
template <typename T>
__device__ __forceinline__ void sf_store4(T* __restrict__ plane, const float* v, int y, int x, int H, int W, bool vec) {
  if (y >= H || x >= W) return;
  T* dst = plane + (int64_t)y * W + x;
  if (vec) {
    Vec<T, 4>::st(dst, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < W) st1(dst + i, v[i]);
  }
}
template <typename T>
__device__ __forceinline__ void sf_load4(const T* __restrict__ plane, float* v, int y, int x, int H, int W, bool vec) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = 0.f;
  if (y >= H || x >= W) return;
  const T* src = plane + (int64_t)y * W + x;
  if (vec) {
    Vec<T, 4>::ld(src, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < W) v[i] = ld1(src + i);
  }
}

// u as the activation dtype stores it (what the backward will read)
template <typename T> __device__ __forceinline__ float sf_stored(float v) { return to_f32(Cvt<T>::from(v)); }

// ------------------------------------------------------------------ forward
// one stencil channel of one tile: u = stencil(h) + bias -> up (optional); GELU: g = gelu_erf(u as stored) -> gp
template <typename T, int KS, int DIL, bool GELU>
__device__ __forceinline__ void sf_fwd_body(float* L, const T* __restrict__ hp, const float* __restrict__ w, float bias, T* __restrict__ up,
                                            T* __restrict__ gp, int H, int W, int ty0, int tx0, bool vec) {
  constexpr int R = DIL * (KS - 1) / 2;
  sf_stage<T, R, false>(L, hp, nullptr, nullptr, H, W, ty0, tx0, vec);
  __syncthreads();
  const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
  float acc[4] = {bias, bias, bias, bias};
#pragma unroll
  for (int dy = 0; dy < KS; ++dy) {
    float win[12];
    sf_window(L + (ty + dy * DIL) * SF_LW + tx, win);
#pragma unroll
    for (int dx = 0; dx < KS; ++dx) {
      const float wv = w[dy * KS + dx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(wv, win[SF_PAD + i + dx * DIL - R], acc[i]);
    }
  }
  if (up) sf_store4<T>(up, acc, ty0 + ty, tx0 + tx, H, W, vec);
  if constexpr (GELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = sf_gelu<T>(sf_stored<T>(acc[i]));
    sf_store4<T>(gp, acc, ty0 + ty, tx0 + tx, H, W, vec);
  }
}

// grid (tiles, S s, B).  MODE SF_FFN: u (optional) and g; MODE SF_LOCAL: u only (g unused).
template <typename T, int MODE>
__global__ __launch_bounds__(SF_THREADS) void sf_fwd_kernel(const T* __restrict__ h, SegPtrs sp, T* __restrict__ u, T* __restrict__ g, int s,
                                                            int H, int W, int tiles_x, int vec) {
  __shared__ __attribute__((aligned(16))) float L[SF_MAXLT];
  const int ch = blockIdx.y, b = blockIdx.z, k = ch / s, j = ch - k * s;
  const int ty0 = (blockIdx.x / tiles_x) * SF_TH, tx0 = (blockIdx.x % tiles_x) * SF_TW;
  const int64_t po = ((int64_t)b * gridDim.y + ch) * H * W;
  const T* hp = h + po;
  T* up = u ? u + po : nullptr;
  T* gp = g ? g + po : nullptr;
  if constexpr (MODE == SF_FFN) {
    if (k == 0) {                                            // identity: u = h
      const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
      float v[4];
      sf_load4<T>(hp, v, ty0 + ty, tx0 + tx, H, W, vec);
      if (up) sf_store4<T>(up, v, ty0 + ty, tx0 + tx, H, W, vec);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = sf_gelu<T>(v[i]);
      sf_store4<T>(gp, v, ty0 + ty, tx0 + tx, H, W, vec);
    } else if (k == 1) {
      sf_fwd_body<T, 3, 1, true>(L, hp, sp.w[1] + j * 9, sp.b[1][j], up, gp, H, W, ty0, tx0, vec);
    } else if (k == 2) {
      sf_fwd_body<T, 5, 1, true>(L, hp, sp.w[2] + j * 25, sp.b[2][j], up, gp, H, W, ty0, tx0, vec);
    } else {
      sf_fwd_body<T, 7, 1, true>(L, hp, sp.w[3] + j * 49, sp.b[3][j], up, gp, H, W, ty0, tx0, vec);
    }
  } else {
    if (k == 0) sf_fwd_body<T, 3, 1, false>(L, hp, sp.w[0] + j * 9, sp.b[0][j], up, nullptr, H, W, ty0, tx0, vec);
    else sf_fwd_body<T, 3, 2, false>(L, hp, sp.w[1] + j * 9, sp.b[1][j], up, nullptr, H, W, ty0, tx0, vec);
  }
}

// ------------------------------------------------------------------ backward
// one stencil channel over the tiles of this workgroup: dh = stencil^T(du), the partial row of dW [ks^2] and db
template <typename T, int KS, int DIL, bool GELU>
__device__ __forceinline__ void sf_bwd_body(float* L, float* red, const T* __restrict__ dp, const T* __restrict__ up, const T* __restrict__ hp,
                                            T* __restrict__ gp, T* __restrict__ dhp, const float* __restrict__ w, float* __restrict__ pw,
                                            float* __restrict__ pb, int H, int W, int tiles_x, int ntiles, int split, int splits,
                                            bool vec) {
  constexpr int R = DIL * (KS - 1) / 2, K2 = KS * KS, NV = K2 + 1;
  float* Ld = L;
  float* Lh = L + SF_MAXLT;
  const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
  float wr[K2], acc[NV];
#pragma unroll
  for (int q = 0; q < K2; ++q) wr[q] = w[q];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.f;
  for (int tile = split; tile < ntiles; tile += splits) {
    const int ty0 = (tile / tiles_x) * SF_TH, tx0 = (tile % tiles_x) * SF_TW;
    __syncthreads();
    sf_stage<T, R, GELU>(Ld, dp, up, gp, H, W, ty0, tx0, vec);
    sf_stage<T, R, false>(Lh, hp, nullptr, nullptr, H, W, ty0, tx0, vec);
    __syncthreads();
    float dc[12], dh[4] = {0.f, 0.f, 0.f, 0.f};
    sf_window(Ld + (ty + R) * SF_LW + tx, dc);               // du at this thread's own pixels: dc[4..7] (zero outside the plane)
    acc[K2] += (dc[4] + dc[5]) + (dc[6] + dc[7]);
#pragma unroll
    for (int dy = 0; dy < KS; ++dy) {
      float wh[12], wd[12];
      sf_window(Lh + (ty + dy * DIL) * SF_LW + tx, wh);
      sf_window(Ld + (ty + 2 * R - dy * DIL) * SF_LW + tx, wd);
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[dy * KS + dx] = fmaf(dc[4 + i], wh[SF_PAD + i + dx * DIL - R], acc[dy * KS + dx]);
          dh[i] = fmaf(wr[dy * KS + dx], wd[SF_PAD + i + R - dx * DIL], dh[i]);
        }
      }
    }
    sf_store4<T>(dhp, dh, ty0 + ty, tx0 + tx, H, W, vec);
  }
  const float tot = block_sum4<NV>(acc, red);
  const int n = threadIdx.x;
  if (n < K2) pw[n] = tot;
  else if (n == K2) pb[0] = tot;
}

// grid (splits, channels, B); row = b splits + split.  MODE SF_FFN: d is dg, u and g as in sf_stage; MODE SF_LOCAL: d is du.
// SEG < 0: every segment in one launch (blockIdx.y is the channel); SEG >= 0: segment SEG alone (blockIdx.y is the channel within
// it).  The FFN runs one launch per segment: as one kernel the four branches together took 256 VGPRs and 40-96 AGPRs, one wave
// per SIMD for every channel; apart, the 7 x 7 branch takes 192 and the others far fewer.
template <typename T, int MODE, int SEG>
__global__ __launch_bounds__(SF_THREADS) void sf_bwd_kernel(const T* __restrict__ d, const T* __restrict__ u, const T* __restrict__ h,
                                                            SegPtrs sp, T* __restrict__ g, T* __restrict__ dh, SegParts parts, int s,
                                                            int H, int W, int tiles_x, int ntiles, int vec) {
  __shared__ __attribute__((aligned(16))) float L[2 * SF_MAXLT];
  __shared__ float red[4 * 50];
  const int split = blockIdx.x, splits = gridDim.x, b = blockIdx.z;
  const int ch = SEG < 0 ? (int)blockIdx.y : SEG * s + (int)blockIdx.y, k = SEG < 0 ? ch / s : SEG, j = ch - k * s;
  const int C = (MODE == SF_FFN ? 4 : 2) * s;
  const int64_t po = ((int64_t)b * C + ch) * H * W, row = (int64_t)b * splits + split;
  const T* dp = d + po;
  const T* hp = h + po;
  T* dhp = dh + po;
  if constexpr (MODE == SF_FFN) {
    const T* up = u + po;
    T* gp = g + po;
    if (k == 0) {                                            // identity: dh = du = dg gelu'(u)
      const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
      for (int tile = split; tile < ntiles; tile += splits) {
        const int y = (tile / tiles_x) * SF_TH + ty, x = (tile % tiles_x) * SF_TW + tx;
        float dv[4], uv[4], gv[4];
        sf_load4<T>(dp, dv, y, x, H, W, vec);
        sf_load4<T>(up, uv, y, x, H, W, vec);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float cdf, pdf;
          sf_gelu_parts<T>(uv[i], cdf, pdf);
          gv[i] = uv[i] * cdf;
          dv[i] *= cdf + uv[i] * pdf;
        }
        sf_store4<T>(gp, gv, y, x, H, W, vec);
        sf_store4<T>(dhp, dv, y, x, H, W, vec);
      }
    } else if (k == 1) {
      float* pr = parts.p[1] + row * s * 10;
      sf_bwd_body<T, 3, 1, true>(L, red, dp, up, hp, gp, dhp, sp.w[1] + j * 9, pr + j * 9, pr + s * 9 + j, H, W, tiles_x, ntiles, split,
                                 splits, vec);
    } else if (k == 2) {
      float* pr = parts.p[2] + row * s * 26;
      sf_bwd_body<T, 5, 1, true>(L, red, dp, up, hp, gp, dhp, sp.w[2] + j * 25, pr + j * 25, pr + s * 25 + j, H, W, tiles_x, ntiles,
                                 split, splits, vec);
    } else {
      float* pr = parts.p[3] + row * s * 50;
      sf_bwd_body<T, 7, 1, true>(L, red, dp, up, hp, gp, dhp, sp.w[3] + j * 49, pr + j * 49, pr + s * 49 + j, H, W, tiles_x, ntiles,
                                 split, splits, vec);
    }
  } else {
    float* pr = parts.p[k] + row * s * 10;
    if (k == 0)
      sf_bwd_body<T, 3, 1, false>(L, red, dp, nullptr, hp, nullptr, dhp, sp.w[0] + j * 9, pr + j * 9, pr + s * 9 + j, H, W, tiles_x,
                                  ntiles, split, splits, vec);
    else
      sf_bwd_body<T, 3, 2, false>(L, red, dp, nullptr, hp, nullptr, dhp, sp.w[1] + j * 9, pr + j * 9, pr + s * 9 + j, H, W, tiles_x,
                                  ntiles, split, splits, vec);
  }
}

// ------------------------------------------------------------------ the plan: the ONE place that decides the launches
enum { SS_PW = 0, SS_GRAM, SS_CS, SS_PART, SS_G, SS_DG, SS_DH, SF_SECTIONS };
struct SfPlan {
  int mode, B, dim, C, S, s, H, W, dtype;          // C = S s channels of the segmented tensor
  int ks[SF_MAX_SEG], halo[SF_MAX_SEG];
  int tiles_x, tiles_y, ntiles, splits;
  int64_t N, rows, part_cols, part_off[SF_MAX_SEG];   // partial rows B splits; columns in all; float offset of segment k's rows
  int kernels_fwd, kernels_bwd, lib_fwd, lib_bwd;
  Sections<SF_SECTIONS> ws;
  Sections<2> saved;                                  // the FFN's blob: h, then u
};

int sf_check(const char* who, int mode, const void* shape, int B, int dim, int H, int W, int dtype, SfPlan* p) {
  MI_CHECK_ARG(shape, "%s: null shape", who);
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "%s: bad dtype %d", who, dtype);
  MI_CHECK_ARG(B >= 1 && B <= 65535, "%s: bad shape B=%d (1..65535)", who, B);
  MI_CHECK_ARG(dim >= 2 && dim <= SF_MAX_DIM, "%s: dim=%d outside the supported 2..%d", who, dim, SF_MAX_DIM);
  MI_CHECK_ARG(dim % 2 == 0, "%s: dim=%d is odd: not covered (the reference's chunk count changes)", who, dim);
  MI_CHECK_ARG(H >= 1 && W >= 1, "%s: bad plane H=%d W=%d", who, H, W);
  memset(p, 0, sizeof(*p));
  p->mode = mode; p->B = B; p->dim = dim; p->H = H; p->W = W; p->dtype = dtype;
  p->s = dim / 2;
  p->S = mode == SF_FFN ? 4 : 2;
  p->C = p->S * p->s;
  p->N = (int64_t)H * W;
  const double elems = (double)B * p->C * (double)p->N;
  MI_CHECK_ARG(elems < 2147483648.0, "%s: B*%d*H*W = %.0f elements, beyond the 2^31 the 1x1 path indexes", who, p->C, elems);
  static const int KS_FFN[4] = {1, 3, 5, 7}, KS_LOC[2] = {3, 3}, DIL_LOC[2] = {1, 2};
  p->tiles_x = cdiv(W, SF_TW); p->tiles_y = cdiv(H, SF_TH); p->ntiles = p->tiles_x * p->tiles_y;
  p->splits = p->ntiles < SF_MAX_SPLITS ? p->ntiles : SF_MAX_SPLITS;
  p->rows = (int64_t)B * p->splits;
  for (int k = 0; k < p->S; ++k) {
    p->ks[k] = mode == SF_FFN ? KS_FFN[k] : KS_LOC[k];
    p->halo[k] = (mode == SF_FFN ? 1 : DIL_LOC[k]) * (p->ks[k] - 1) / 2;
    p->part_off[k] = p->rows * p->part_cols;
    if (p->ks[k] > 1) p->part_cols += (int64_t)p->s * (p->ks[k] * p->ks[k] + 1);
  }
  Sections<SF_SECTIONS>& ws = p->ws;
  if (mode == SF_FFN) {
    const int C = p->C, dt = dtype;
    const int64_t N = p->N;
    ws.put(SS_PW, max_of({pw_ws_bytes(probe1x1(dim, C, false, B, N, dt)), pw_ws_bytes(probe1x1(C, dim, false, B, N, dt)),
                          pw_ws_bytes(probe1x1(dim, C, true, B, N, dt)), pw_ws_bytes(probe1x1(C, dim, true, B, N, dt))}));
    ws.put(SS_GRAM, max_of({gram_ws_bytes(probe_wgrad(dim, C, B, N, dt)), gram_ws_bytes(probe_wgrad(C, dim, B, N, dt))}));
    ws.put(SS_CS, chan_sum_workspace(C, N));
    ws.put(SS_PART, (size_t)(p->rows * p->part_cols) * sizeof(float));
    const size_t plane = (size_t)B * C * N * dtype_size(dt);
    ws.put(SS_G, plane);
    ws.put(SS_DG, plane);                                    // inference: h
    ws.put(SS_DH, plane);
    p->saved.put(0, plane); p->saved.put(1, plane);
    p->kernels_fwd = 1; p->kernels_bwd = 7; p->lib_fwd = 2; p->lib_bwd = 6;
  } else {
    ws.put(SS_PART, (size_t)(p->rows * p->part_cols) * sizeof(float));
    p->kernels_fwd = 1; p->kernels_bwd = 3;
  }
  return MI_OK;
}
int sf_check(const char* who, const mi_sfh_ffn_shape* s, SfPlan* p) {
  return sf_check(who, SF_FFN, s, s ? s->B : 0, s ? s->dim : 0, s ? s->H : 0, s ? s->W : 0, s ? s->dtype : 0, p);
}
int sf_check(const char* who, const mi_sfh_local_shape* s, SfPlan* p) {
  return sf_check(who, SF_LOCAL, s, s ? s->B : 0, s ? s->dim : 0, s ? s->H : 0, s ? s->W : 0, s ? s->dtype : 0, p);
}

// 23 scalars (tile, segments, halos, tiles, partial rows, launch counts, LDS bytes forward / backward, threads), the SS_* sections
// from [24]; [62]: the offset of u in the saved blob (the format: plan_report, internal.h)
int sf_plan_out(const SfPlan& p, int64_t* out) {
  return plan_report<24>(out, {SF_TW, SF_TH, p.S, p.s, p.halo[0], p.halo[1], p.halo[2], p.halo[3], p.tiles_x, p.tiles_y, p.ntiles, p.C,
                               p.B, p.splits, p.rows, p.part_cols, p.kernels_fwd, p.kernels_bwd, p.lib_fwd, p.lib_bwd,
                               (int64_t)(SF_MAXLT * sizeof(float)), (int64_t)((2 * SF_MAXLT + 4 * 50) * sizeof(float)), SF_THREADS},
                         p.ws, {(int64_t)p.ws.total, (int64_t)p.saved.total, (int64_t)p.saved.off[1]});
}

// rows are 4 wide where every row of every plane starts on a 16-byte boundary of its dtype's 4-element chunk
bool sf_vec(const SfPlan& p, std::initializer_list<const void*> ptrs) {
  if (p.W % 4) return false;
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return false;
  return true;
}

int sf_fwd(const SfPlan& p, const void* h, const SegPtrs& sp, void* u, void* g, hipStream_t st) {
  const dim3 grid(p.ntiles, p.C, p.B);
  const int vec = sf_vec(p, {h, u, g});
  return with_dtype(p.dtype, "sfh_segmented_fwd", [&](auto tag) {
    using T = decltype(tag);
    if (p.mode == SF_FFN)
      hipLaunchKernelGGL((sf_fwd_kernel<T, SF_FFN>), grid, dim3(SF_THREADS), 0, st, (const T*)h, sp, (T*)u, (T*)g, p.s, p.H, p.W,
                         p.tiles_x, vec);
    else
      hipLaunchKernelGGL((sf_fwd_kernel<T, SF_LOCAL>), grid, dim3(SF_THREADS), 0, st, (const T*)h, sp, (T*)u, (T*)g, p.s, p.H, p.W,
                         p.tiles_x, vec);
  });
}

// gw / gb: the gradient buffers of segment k (unused for an identity segment)
int sf_bwd(const SfPlan& p, const void* d, const void* u, const void* h, const SegPtrs& sp, void* g, void* dh, float* part,
           float* const* gw, float* const* gb, int accumulate, hipStream_t st) {
  const int vec = sf_vec(p, {d, u, h, g, dh});
  SegParts parts;
  for (int k = 0; k < SF_MAX_SEG; ++k) parts.p[k] = part + p.part_off[k];
  auto launch = [&](auto tag, auto mode, auto seg, int channels) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((sf_bwd_kernel<T, decltype(mode)::value, decltype(seg)::value>), dim3(p.splits, channels, p.B), dim3(SF_THREADS), 0,
                       st, (const T*)d, (const T*)u, (const T*)h, sp, (T*)g, (T*)dh, parts, p.s, p.H, p.W, p.tiles_x, p.ntiles, vec);
    MI_LAUNCH_CHECK();
    return MI_OK;
  };
  using FfnMode = std::integral_constant<int, SF_FFN>;
  using LocalMode = std::integral_constant<int, SF_LOCAL>;
  MI_TRY(with_dtype(p.dtype, "sfh_segmented_bwd", [&](auto tag) -> int {
    if (p.mode == SF_LOCAL) return launch(tag, LocalMode{}, std::integral_constant<int, -1>{}, p.C);
    MI_TRY(launch(tag, FfnMode{}, std::integral_constant<int, 0>{}, p.s));
    MI_TRY(launch(tag, FfnMode{}, std::integral_constant<int, 1>{}, p.s));
    MI_TRY(launch(tag, FfnMode{}, std::integral_constant<int, 2>{}, p.s));
    return launch(tag, FfnMode{}, std::integral_constant<int, 3>{}, p.s);
  }));
  for (int k = 0; k < p.S; ++k) {
    if (p.ks[k] == 1) continue;
    const int64_t k2 = p.ks[k] * p.ks[k], cols = p.s * (k2 + 1);
    MI_TRY(launch_reduce_rows(parts.p[k], gw[k], p.rows, cols, cols, accumulate, 1.0f, st, nullptr, gb[k], p.s * k2));
  }
  return MI_OK;
}

}  // namespace
}  // namespace mi

using namespace mi;

// ------------------------------------------------------------------ FFN
extern "C" size_t mi_sfh_ffn_workspace(const mi_sfh_ffn_shape* s) {
  SfPlan p;
  return sf_check("sfh_ffn_workspace", s, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" size_t mi_sfh_ffn_saved_bytes(const mi_sfh_ffn_shape* s) {
  SfPlan p;
  return sf_check("sfh_ffn_saved_bytes", s, &p) == MI_OK ? p.saved.total : 0;
}
extern "C" int mi_sfh_ffn_plan(const mi_sfh_ffn_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "sfh_ffn_plan: null pointer");
  SfPlan p;
  MI_TRY(sf_check("sfh_ffn_plan", s, &p));
  return sf_plan_out(p, out);
}

static SegPtrs ffn_seg(const mi_sfh_ffn_params* pr) {
  return SegPtrs{{nullptr, pr->c1_w, pr->c2_w, pr->c3_w}, {nullptr, pr->c1_b, pr->c2_b, pr->c3_b}};
}
static bool ffn_params_ok(const mi_sfh_ffn_params* pr) {
  return pr && pr->init_w && pr->init_b && pr->c1_w && pr->c1_b && pr->c2_w && pr->c2_b && pr->c3_w && pr->c3_b && pr->fina_w && pr->fina_b;
}

extern "C" int mi_sfh_ffn_fwd(const mi_sfh_ffn_shape* s, const mi_sfh_ffn_params* pr, const void* x, void* out, void* saved, void* ws,
                              void* stream) {
  SfPlan p;
  MI_TRY(sf_check("sfh_ffn_fwd", s, &p));
  MI_CHECK_ARG(ffn_params_ok(pr) && x && out && ws, "sfh_ffn_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<SF_SECTIONS>& w = p.ws;
  void* h = saved ? saved : w.at<void>(ws, SS_DG);
  void* u = saved ? p.saved.at<void>(saved, 1) : nullptr;
  void* g = w.at(ws, SS_G);
  const mi_pw_desc d1 = conv1x1(x, p.dim, pr->init_w, false, p.dim, pr->init_b, nullptr, h, p.C, p.B, p.N, p.dtype);      // SFHformer.py:109
  MI_TRY(mi_pw_gemm(&d1, w.at(ws, SS_PW), st));
  MI_TRY(sf_fwd(p, h, ffn_seg(pr), u, g, st));                                                                              // :110-115
  const mi_pw_desc d2 = conv1x1(g, p.C, pr->fina_w, false, p.C, pr->fina_b, nullptr, out, p.dim, p.B, p.N, p.dtype);       // :116
  return mi_pw_gemm(&d2, w.at(ws, SS_PW), st);
}

extern "C" int mi_sfh_ffn_bwd(const mi_sfh_ffn_shape* s, const mi_sfh_ffn_params* pr, const void* x, const void* dout, void* dx,
                              const mi_sfh_ffn_grads* gr, const void* saved, void* ws, void* stream) {
  SfPlan p;
  MI_TRY(sf_check("sfh_ffn_bwd", s, &p));
  MI_CHECK_ARG(ffn_params_ok(pr) && x && dout && dx && gr && saved && ws, "sfh_ffn_bwd: null pointer");
  MI_CHECK_ARG(gr->init_w && gr->init_b && gr->c1_w && gr->c1_b && gr->c2_w && gr->c2_b && gr->c3_w && gr->c3_b && gr->fina_w &&
               gr->fina_b, "sfh_ffn_bwd: null gradient buffer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<SF_SECTIONS>& w = p.ws;
  const int acc = gr->accumulate ? 1 : 0;
  const void* h = saved;
  const void* u = p.saved.at<void>(saved, 1);
  void* g = w.at(ws, SS_G);
  void* dg = w.at(ws, SS_DG);
  void* dh = w.at(ws, SS_DH);
  float* part = w.at(ws, SS_PART);
  MI_TRY(launch_chan_sum(dout, gr->fina_b, p.B, p.dim, p.N, p.dtype, acc, w.at(ws, SS_CS), st));
  const mi_pw_desc d2 = conv1x1(dout, p.dim, pr->fina_w, true, p.C, nullptr, nullptr, dg, p.C, p.B, p.N, p.dtype);
  MI_TRY(mi_pw_gemm(&d2, w.at(ws, SS_PW), st));
  float* const gw[SF_MAX_SEG] = {nullptr, gr->c1_w, gr->c2_w, gr->c3_w};
  float* const gb[SF_MAX_SEG] = {nullptr, gr->c1_b, gr->c2_b, gr->c3_b};
  MI_TRY(sf_bwd(p, dg, u, h, ffn_seg(pr), g, dh, part, gw, gb, acc, st));
  const mi_gram_desc g2 = wgrad_gram(dout, p.dim, g, p.C, p.B, p.N, p.dtype, gr->fina_w, acc);
  MI_TRY(mi_gram(&g2, w.at(ws, SS_GRAM), st));
  return conv1x1_bwd_input(dh, p.C, x, p.dim, pr->init_w, gr->init_w, gr->init_b, dx, p.B, p.N, p.dtype, acc, w.at(ws, SS_GRAM),
                           w.at(ws, SS_CS), w.at(ws, SS_PW), st, false);
}

// ------------------------------------------------------------------ TokenMixer_For_Local
extern "C" size_t mi_sfh_local_workspace(const mi_sfh_local_shape* s) {
  SfPlan p;
  return sf_check("sfh_local_workspace", s, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" int mi_sfh_local_plan(const mi_sfh_local_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "sfh_local_plan: null pointer");
  SfPlan p;
  MI_TRY(sf_check("sfh_local_plan", s, &p));
  return sf_plan_out(p, out);
}
static bool local_params_ok(const mi_sfh_local_params* pr) { return pr && pr->cd1_w && pr->cd1_b && pr->cd2_w && pr->cd2_b; }

extern "C" int mi_sfh_local_fwd(const mi_sfh_local_shape* s, const mi_sfh_local_params* pr, const void* x, void* out, void* ws,
                                void* stream) {
  SfPlan p;
  MI_TRY(sf_check("sfh_local_fwd", s, &p));
  MI_CHECK_ARG(local_params_ok(pr) && x && out && ws, "sfh_local_fwd: null pointer");
  const SegPtrs sp = {{pr->cd1_w, pr->cd2_w, nullptr, nullptr}, {pr->cd1_b, pr->cd2_b, nullptr, nullptr}};
  return sf_fwd(p, x, sp, out, nullptr, (hipStream_t)stream);                                                               // :135-138
}

extern "C" int mi_sfh_local_bwd(const mi_sfh_local_shape* s, const mi_sfh_local_params* pr, const void* x, const void* dout, void* dx,
                                const mi_sfh_local_grads* gr, void* ws, void* stream) {
  SfPlan p;
  MI_TRY(sf_check("sfh_local_bwd", s, &p));
  MI_CHECK_ARG(local_params_ok(pr) && x && dout && dx && gr && ws, "sfh_local_bwd: null pointer");
  MI_CHECK_ARG(gr->cd1_w && gr->cd1_b && gr->cd2_w && gr->cd2_b, "sfh_local_bwd: null gradient buffer");
  const SegPtrs sp = {{pr->cd1_w, pr->cd2_w, nullptr, nullptr}, {pr->cd1_b, pr->cd2_b, nullptr, nullptr}};
  float* const gw[SF_MAX_SEG] = {gr->cd1_w, gr->cd2_w, nullptr, nullptr};
  float* const gb[SF_MAX_SEG] = {gr->cd1_b, gr->cd2_b, nullptr, nullptr};
  return sf_bwd(p, dout, nullptr, x, sp, nullptr, dx, p.ws.at(ws, SS_PART), gw, gb, gr->accumulate ? 1 : 0,
                (hipStream_t)stream);
}
