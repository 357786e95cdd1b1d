// The pixel-space loss terms of the reference's training steps besides L1 and the FFT loss, each with d loss / d pred from the
// same library call (MoCE-IR-main/src/utils/loss_utils.py: SSIMloss / SSIM :35-55, FocalL1Loss :100-136, EdgeLoss :155-190).
// House rules of mi_fft_l1_loss: fp32 arithmetic on inputs widened on load, dpred rounded once, the loss a device float that is
// overwritten, the caller's workspace, no atomics (one partial per workgroup, summed in a fixed order by ONE finishing
// workgroup), no allocation, no host synchronisation.
//
//   focal   one flat pass: a = |d| / alpha, f = log1p(a + epsilon)^gamma a, df/dd = sign(d) / alpha (L^gamma + gamma a L^(gamma-1)
//           / (1 + a + epsilon)); sign(0) = 0, so a tie's gradient is an exact 0 also where L^(gamma-1) overflows.
//   edge    L = I - G D G, G the 5x5 blur over a replicate-padded plane, D = 4 on even (row, col) and 0 elsewhere.  One tiled
//           kernel template does both e = L d and L^T s: the plane tile with a 4-pixel halo goes to LDS (zero outside the plane),
//           the middle product D G over a 2-pixel halo, then the outer G.  Replicate padding is folded into per-axis tap weights
//           ed_w(t, s) = sum of k[a] with clamp(t + a - 2) == s, so a border pixel collects the taps clamped onto it; the adjoint
//           swaps the two arguments and is a gather as well.
//   ssim    two kernels with three fp32 maps between them: the map kernel takes a 32 x 32 tile of the (H-10) x (W-10) map from a
//           42 x 42 input patch (separable 11-tap window: rows into LDS, then columns), sums S and stores Ga, Gb, Gc; the gradient
//           kernel runs the full (zero-extended) correlation of the three maps over a 32 x 32 tile of the image and combines
//           them with x and y.
#include <limits.h>

#include "internal.h"

namespace mi {
namespace {

constexpr int LS_THREADS = 256;
constexpr int FO_MAX_BLOCKS = 1024;                     // focal: partials (a capped grid-stride grid)
constexpr int ED_T = 32, ED_IN = ED_T + 8, ED_MID = ED_T + 4;   // edge: output tile, with the 4- and the 2-pixel halo
constexpr int SS_T = MI_SSIM_TILE, SS_WIN = 11, SS_IN = SS_T + SS_WIN - 1;

// lanes, then the four waves, in a fixed order; every thread of the workgroup must call it
__device__ __forceinline__ float ls_block_sum(float v, float* sred) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}

// One workgroup: m = inv_count * sum of the partials (thread t takes partials t, t + 256, ... in order).
// ssim: loss[0] = weight (1 - m), loss[1] = m;  otherwise loss[0] = weight m.
__global__ __launch_bounds__(LS_THREADS) void ls_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ loss,
                                                               float inv_count, float weight, int ssim) {
  __shared__ float sred[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += LS_THREADS) acc += part[i];
  const float m = ls_block_sum(acc, sred) * inv_count;
  if (threadIdx.x == 0) {
    if (ssim) { loss[0] = weight * (1.f - m); loss[1] = m; }
    else loss[0] = weight * m;
  }
}

int ls_finish(const float* part, int n, float* loss, double count, float weight, int ssim, hipStream_t st) {
  ProfScope ps(st, K_L1, (double)n * 4, (double)n);
  hipLaunchKernelGGL(ls_finish_kernel, dim3(1), dim3(LS_THREADS), 0, st, part, n, loss, (float)(1.0 / count), weight, ssim);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------------------------ focal L1
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void focal_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                           T* __restrict__ dpred, float* __restrict__ part, int64_t n, float gamma,
                                                           float eps, float alpha, float gscale) {
  __shared__ float sred[4];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * LS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x; i < n; i += stride) {
    const float d = ld1(pred + i) - ld1(target + i);
    const float a = fabsf(d) / alpha;
    const float L = log1pf(a + eps);
    const float w = powf(L, gamma);
    acc += w * a;
    if (dpred) {
      float g = 0.f;                                    // sign(0) = 0: an exact zero, whatever L^(gamma-1) is at a = 0
      if (d != 0.f) g = copysignf((w + a * gamma * (w / L) / (1.f + a + eps)) * gscale, d);
      st1(dpred + i, g);
    }
  }
  const float tot = ls_block_sum(acc, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------------------------------------- edge
// Weight the replicate-padded 5-tap blur k = [.05 .25 .4 .25 .05] puts on source s for output t on an axis of n pixels
// (0 <= t, s < n): every tap whose clamped position is s.
__device__ __forceinline__ float ed_w(int t, int s, int n) {
  float w = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int c = min(max(t + a - 2, 0), n - 1);
    const float k = a == 2 ? .4f : ((a == 1 || a == 3) ? .25f : .05f);
    if (c == s) w += k;
  }
  return w;
}

// FWD: in = pred - target, r = L in; the criterion's sum goes to part[workgroup], and map (if given) gets what the adjoint
// starts from (r for l2, sign(r) for l1).   !FWD: in = map, dpred = gscale * L^T in.
template <typename T, bool FWD>
__global__ __launch_bounds__(LS_THREADS) void edge_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                          float* __restrict__ map, T* __restrict__ dpred, float* __restrict__ part,
                                                          int H, int W, int tiles_x, int tiles_y, int criterion, float gscale) {
  __shared__ float sIn[ED_IN][ED_IN + 1];
  __shared__ float sMid[ED_MID][ED_MID + 1];
  __shared__ float sWy[ED_MID][5], sWx[ED_MID][5];     // tap weights of the targets y0 - 2 + i / x0 - 2 + i
  __shared__ float sred[4];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int64_t base = (int64_t)(bid / tiles_y) * H * W;
  const int y0 = ty * ED_T, x0 = tx * ED_T;

  for (int e = tid; e < ED_IN * ED_IN; e += LS_THREADS) {
    const int i = e / ED_IN, j = e - i * ED_IN;
    const int gy = y0 - 4 + i, gx = x0 - 4 + j;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int64_t o = base + (int64_t)gy * W + gx;
      v = FWD ? ld1(pred + o) - ld1(target + o) : map[o];
    }
    sIn[i][j] = v;
  }
  for (int e = tid; e < 2 * ED_MID * 5; e += LS_THREADS) {
    const int axis = e / (ED_MID * 5), r = e - axis * (ED_MID * 5);
    const int i = r / 5, a = r - i * 5;
    const int n = axis ? W : H;
    const int t = (axis ? x0 : y0) - 2 + i, s = t + a - 2;
    float w = 0.f;
    if (t >= 0 && t < n && s >= 0 && s < n) w = FWD ? ed_w(t, s, n) : ed_w(s, t, n);
    if (axis) sWx[i][a] = w; else sWy[i][a] = w;
  }
  __syncthreads();

  for (int e = tid; e < ED_MID * ED_MID; e += LS_THREADS) {     // 4 * (blur) on the even grid, zero elsewhere and outside
    const int i = e / ED_MID, j = e - i * ED_MID;
    const int gy = y0 - 2 + i, gx = x0 - 2 + j;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W && !(gy & 1) && !(gx & 1)) {
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        float h = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) h += sWx[j][b] * sIn[i + a][j + b];
        v += sWy[i][a] * h;
      }
      v *= 4.f;
    }
    sMid[i][j] = v;
  }
  __syncthreads();

  float acc = 0.f;
  for (int e = tid; e < ED_T * ED_T; e += LS_THREADS) {
    const int i = e / ED_T, j = e - i * ED_T;
    const int gy = y0 + i, gx = x0 + j;
    if (gy >= H || gx >= W) continue;
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      float h = 0.f;
#pragma unroll
      for (int b = 0; b < 5; ++b) h += sWx[j + 2][b] * sMid[i + a][j + b];
      v += sWy[i + 2][a] * h;
    }
    const float r = sIn[i + 4][j + 4] - v;
    const int64_t o = base + (int64_t)gy * W + gx;
    if (FWD) {
      acc += criterion ? fabsf(r) : r * r;
      if (map) map[o] = criterion ? (float)((r > 0.f) - (r < 0.f)) : r;
    } else {
      st1(dpred + o, gscale * r);
    }
  }
  if (FWD) {
    const float tot = ls_block_sum(acc, sred);
    if (tid == 0) part[blockIdx.x] = tot;
  }
}

struct EdPlan { int P, tiles_x, tiles_y, grid; size_t off_map, off_part, total; };
bool ed_plan(int B, int C, int H, int W, EdPlan* p) {
  *p = EdPlan{};
  if (B <= 0 || C <= 0 || H < 2 || W < 2) return false;
  const int64_t P = (int64_t)B * C;
  const int tx = cdiv(W, ED_T), ty = cdiv(H, ED_T);
  const int64_t grid = P * tx * ty;
  if (P > INT_MAX || grid > INT_MAX) return false;
  p->P = (int)P; p->tiles_x = tx; p->tiles_y = ty; p->grid = (int)grid;
  p->off_map = 0;
  p->off_part = fbytes((size_t)P * H * W);
  p->total = p->off_part + fbytes((size_t)grid);
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------- ssim
struct SsWin { float g[SS_WIN]; };

// pytorch_msssim.ssim's window: exp(-(i - 5)^2 / (2 1.5^2)), normalised to sum 1
SsWin ss_window() {
  double g[SS_WIN], s = 0.0;
  for (int i = 0; i < SS_WIN; ++i) { g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += g[i]; }
  SsWin w;
  for (int i = 0; i < SS_WIN; ++i) w.g[i] = (float)(g[i] / s);
  return w;
}

// One 32 x 32 tile of the map per workgroup: part[workgroup] = the tile's sum of S; ga / gb / gc (if given) [P][Hm][Wm].
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void ssim_map_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                              float* __restrict__ ga, float* __restrict__ gb, float* __restrict__ gc,
                                                              float* __restrict__ part, int H, int W, int Hm, int Wm, int tiles_x,
                                                              int tiles_y, const SsWin win, float C1, float C2) {
  __shared__ float sx[SS_IN][SS_IN + 1], sy[SS_IN][SS_IN + 1];
  __shared__ float sh[5][SS_IN][SS_T + 1];              // rows filtered: x, y, xx, yy, xy
  __shared__ float sred[4];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int64_t plane = bid / tiles_y;
  const int y0 = ty * SS_T, x0 = tx * SS_T;

  for (int e = tid; e < SS_IN * SS_IN; e += LS_THREADS) {      // map (y, x) reads the image at (y .. y + 10, x .. x + 10)
    const int i = e / SS_IN, j = e - i * SS_IN;
    const int gy = y0 + i, gx = x0 + j;
    float vx = 0.f, vy = 0.f;
    if (gy < H && gx < W) {
      const int64_t o = (plane * H + gy) * W + gx;
      vx = ld1(pred + o); vy = ld1(target + o);
    }
    sx[i][j] = vx; sy[i][j] = vy;
  }
  __syncthreads();
  for (int e = tid; e < SS_IN * SS_T; e += LS_THREADS) {
    const int i = e / SS_T, j = e - i * SS_T;
    float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const float g = win.g[k], x = sx[i][j + k], y = sy[i][j + k];
      hx += g * x; hy += g * y; hxx += g * (x * x); hyy += g * (y * y); hxy += g * (x * y);
    }
    sh[0][i][j] = hx; sh[1][i][j] = hy; sh[2][i][j] = hxx; sh[3][i][j] = hyy; sh[4][i][j] = hxy;
  }
  __syncthreads();
  float acc = 0.f;
  for (int e = tid; e < SS_T * SS_T; e += LS_THREADS) {
    const int i = e / SS_T, j = e - i * SS_T;
    const int my = y0 + i, mx = x0 + j;
    if (my >= Hm || mx >= Wm) continue;
    float mu1 = 0.f, mu2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const float g = win.g[k];
      mu1 += g * sh[0][i + k][j]; mu2 += g * sh[1][i + k][j];
      exx += g * sh[2][i + k][j]; eyy += g * sh[3][i + k][j]; exy += g * sh[4][i + k][j];
    }
    const float s1 = exx - mu1 * mu1, s2 = eyy - mu2 * mu2, s12 = exy - mu1 * mu2;
    const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2;
    const float B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s1 + s2 + C2;
    const float rB = 1.f / (B1 * B2);
    const float S = A1 * A2 * rB;
    acc += S;
    if (ga) {
      const float dmu = 2.f * mu2 * A2 * rB - 2.f * mu1 * S / B1;
      const float dsg = -S / B2, ds12 = 2.f * A1 * rB;
      const int64_t o = (plane * Hm + my) * Wm + mx;
      ga[o] = dmu - 2.f * mu1 * dsg - mu2 * ds12;
      gb[o] = 2.f * dsg;
      gc[o] = ds12;
    }
  }
  const float tot = ls_block_sum(acc, sred);
  if (tid == 0) part[blockIdx.x] = tot;
}

// One 32 x 32 tile of the image per workgroup: dpred = gscale (G(ga) + x G(gb) + y G(gc)), G the full correlation
// G(M)[y][x] = sum_ij g[i] g[j] M[y - i][x - j] with M zero outside the map.
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void ssim_grad_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                               const float* __restrict__ ga, const float* __restrict__ gb,
                                                               const float* __restrict__ gc, T* __restrict__ dpred, int H, int W,
                                                               int Hm, int Wm, int tiles_x, int tiles_y, const SsWin win,
                                                               float gscale) {
  __shared__ float sm[3][SS_IN][SS_IN + 1];             // maps at rows y0 - 10 + r, columns x0 - 10 + c
  __shared__ float sh[3][SS_IN][SS_T + 1];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int64_t plane = bid / tiles_y;
  const int y0 = ty * SS_T, x0 = tx * SS_T;

  for (int e = tid; e < SS_IN * SS_IN; e += LS_THREADS) {
    const int r = e / SS_IN, c = e - r * SS_IN;
    const int my = y0 - (SS_WIN - 1) + r, mx = x0 - (SS_WIN - 1) + c;
    float a = 0.f, b = 0.f, d = 0.f;
    if (my >= 0 && my < Hm && mx >= 0 && mx < Wm) {
      const int64_t o = (plane * Hm + my) * Wm + mx;
      a = ga[o]; b = gb[o]; d = gc[o];
    }
    sm[0][r][c] = a; sm[1][r][c] = b; sm[2][r][c] = d;
  }
  __syncthreads();
  for (int e = tid; e < SS_IN * SS_T; e += LS_THREADS) {
    const int r = e / SS_T, j = e - r * SS_T;
    float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {                  // column x0 + j - k sits at c = j + 10 - k
      const float g = win.g[k];
      a += g * sm[0][r][j + SS_WIN - 1 - k]; b += g * sm[1][r][j + SS_WIN - 1 - k]; d += g * sm[2][r][j + SS_WIN - 1 - k];
    }
    sh[0][r][j] = a; sh[1][r][j] = b; sh[2][r][j] = d;
  }
  __syncthreads();
  for (int e = tid; e < SS_T * SS_T; e += LS_THREADS) {
    const int i = e / SS_T, j = e - i * SS_T;
    const int gy = y0 + i, gx = x0 + j;
    if (gy >= H || gx >= W) continue;
    float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const float g = win.g[k];
      a += g * sh[0][i + SS_WIN - 1 - k][j]; b += g * sh[1][i + SS_WIN - 1 - k][j]; d += g * sh[2][i + SS_WIN - 1 - k][j];
    }
    const int64_t o = (plane * H + gy) * W + gx;
    st1(dpred + o, gscale * (a + ld1(pred + o) * b + ld1(target + o) * d));
  }
}

struct SsPlan { int P, Hm, Wm, mtx, mty, grid_map, itx, ity, grid_grad; size_t off[4], total; };
bool ss_plan(int B, int C, int H, int W, SsPlan* p) {
  *p = SsPlan{};
  if (B <= 0 || C <= 0 || H < SS_WIN || W < SS_WIN) return false;
  const int64_t P = (int64_t)B * C;
  p->Hm = H - SS_WIN + 1; p->Wm = W - SS_WIN + 1;
  p->mtx = cdiv(p->Wm, SS_T); p->mty = cdiv(p->Hm, SS_T);
  p->itx = cdiv(W, SS_T); p->ity = cdiv(H, SS_T);
  const int64_t g1 = P * p->mtx * p->mty, g2 = P * p->itx * p->ity;
  if (P > INT_MAX || g1 > INT_MAX || g2 > INT_MAX) return false;
  p->P = (int)P; p->grid_map = (int)g1; p->grid_grad = (int)g2;
  const size_t m = fbytes((size_t)P * p->Hm * p->Wm);
  p->off[0] = 0; p->off[1] = m; p->off[2] = 2 * m; p->off[3] = 3 * m;
  p->total = 3 * m + fbytes((size_t)g1);
  return true;
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" size_t mi_focal_l1_workspace(int64_t n) { return n > 0 ? fbytes(FO_MAX_BLOCKS) : 0; }

extern "C" int mi_focal_l1_loss(const void* pred, const void* target, void* dpred, float* loss, int64_t n, float gamma,
                                float epsilon, float alpha, float scale, int dtype, void* ws, void* stream) {
  MI_CHECK_ARG(pred && target && loss && ws, "focal_l1_loss: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "focal_l1_loss: bad dtype %d", dtype);
  MI_CHECK_ARG(n > 0, "focal_l1_loss: bad element count %lld", (long long)n);
  MI_CHECK_ARG(alpha > 0.f, "focal_l1_loss: alpha must be > 0 (got %g)", (double)alpha);
  MI_CHECK_ARG(gamma >= 0.f && epsilon >= 0.f, "focal_l1_loss: gamma and epsilon must be >= 0 (got %g, %g)", (double)gamma,
               (double)epsilon);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const int blocks = cdiv_cap(n, LS_THREADS * 8, FO_MAX_BLOCKS);
  const float gscale = (float)((double)scale / ((double)n * (double)alpha));
  MI_TRY(with_dtype(dtype, "focal_l1_loss", [&](auto tag) -> int {
    using T = decltype(tag);
    ProfScope ps(st, K_L1, (double)n * dtype_size(dtype) * (dpred ? 3 : 2), (double)n * 40);
    hipLaunchKernelGGL((focal_kernel<T>), dim3(blocks), dim3(LS_THREADS), 0, st, (const T*)pred, (const T*)target, (T*)dpred,
                       part, n, gamma, epsilon, alpha, gscale);
    MI_LAUNCH_CHECK();
    return MI_OK;
  }));
  return ls_finish(part, blocks, loss, (double)n, scale, 0, st);
}

extern "C" size_t mi_edge_loss_workspace(int B, int C, int H, int W) {
  EdPlan p;
  return ed_plan(B, C, H, W, &p) ? p.total : 0;
}

extern "C" int mi_edge_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                            float loss_weight, int criterion, int dtype, void* ws, void* stream) {
  MI_CHECK_ARG(pred && target && loss && ws, "edge_loss: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "edge_loss: bad dtype %d", dtype);
  MI_CHECK_ARG(B > 0 && C > 0, "edge_loss: bad shape B=%d C=%d", B, C);
  MI_CHECK_ARG(H >= 2 && W >= 2, "edge_loss: H=%d W=%d below the supported 2 x 2", H, W);
  MI_CHECK_ARG(criterion == 0 || criterion == 1, "edge_loss: bad criterion %d (0: l2, 1: l1)", criterion);
  EdPlan p;
  MI_CHECK_ARG(ed_plan(B, C, H, W, &p), "edge_loss: too many planes or tiles (B=%d C=%d H=%d W=%d)", B, C, H, W);
  hipStream_t st = (hipStream_t)stream;
  float* map = (float*)((char*)ws + p.off_map);
  float* part = (float*)((char*)ws + p.off_part);
  const double N = (double)p.P * H * W;
  const float gscale = (float)((double)loss_weight * (criterion ? 1.0 : 2.0) / N);
  MI_TRY(with_dtype(dtype, "edge_loss", [&](auto tag) -> int {
    using T = decltype(tag);
    ProfScope ps(st, K_L1, N * (2 * dtype_size(dtype) + (dpred ? 4 : 0)), N * 100);
    hipLaunchKernelGGL((edge_kernel<T, true>), dim3(p.grid), dim3(LS_THREADS), 0, st, (const T*)pred, (const T*)target,
                       dpred ? map : (float*)nullptr, (T*)nullptr, part, H, W, p.tiles_x, p.tiles_y, criterion, 0.f);
    MI_LAUNCH_CHECK();
    return MI_OK;
  }));
  MI_TRY(ls_finish(part, p.grid, loss, N, loss_weight, 0, st));
  if (!dpred) return MI_OK;
  return with_dtype(dtype, "edge_loss", [&](auto tag) -> int {
    using T = decltype(tag);
    ProfScope ps(st, K_L1, N * (4 + dtype_size(dtype)), N * 100);
    hipLaunchKernelGGL((edge_kernel<T, false>), dim3(p.grid), dim3(LS_THREADS), 0, st, (const T*)nullptr, (const T*)nullptr, map,
                       (T*)dpred, (float*)nullptr, H, W, p.tiles_x, p.tiles_y, criterion, gscale);
    MI_LAUNCH_CHECK();
    return MI_OK;
  });
}

extern "C" size_t mi_ssim_loss_workspace(int B, int C, int H, int W) {
  SsPlan p;
  return ss_plan(B, C, H, W, &p) ? p.total : 0;
}

extern "C" int mi_ssim_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                            float loss_weight, float data_range, int dtype, void* ws, void* stream) {
  MI_CHECK_ARG(pred && target && loss && ws, "ssim_loss: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "ssim_loss: bad dtype %d", dtype);
  MI_CHECK_ARG(B > 0 && C > 0, "ssim_loss: bad shape B=%d C=%d", B, C);
  MI_CHECK_ARG(H >= SS_WIN && W >= SS_WIN, "ssim_loss: H=%d W=%d below the %d x %d window", H, W, SS_WIN, SS_WIN);
  MI_CHECK_ARG(data_range > 0.f, "ssim_loss: data_range must be > 0 (got %g)", (double)data_range);
  SsPlan p;
  MI_CHECK_ARG(ss_plan(B, C, H, W, &p), "ssim_loss: too many planes or tiles (B=%d C=%d H=%d W=%d)", B, C, H, W);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* ga = (float*)(base + p.off[0]); float* gb = (float*)(base + p.off[1]); float* gc = (float*)(base + p.off[2]);
  float* part = (float*)(base + p.off[3]);
  const SsWin win = ss_window();
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  const double Nm = (double)p.P * p.Hm * p.Wm, N = (double)p.P * H * W;
  const bool want = dpred != nullptr;
  MI_TRY(with_dtype(dtype, "ssim_loss", [&](auto tag) -> int {
    using T = decltype(tag);
    ProfScope ps(st, K_L1, N * 2 * dtype_size(dtype) + (want ? Nm * 12 : 0), Nm * 200);
    hipLaunchKernelGGL((ssim_map_kernel<T>), dim3(p.grid_map), dim3(LS_THREADS), 0, st, (const T*)pred, (const T*)target,
                       want ? ga : (float*)nullptr, gb, gc, part, H, W, p.Hm, p.Wm, p.mtx, p.mty, win, C1, C2);
    MI_LAUNCH_CHECK();
    return MI_OK;
  }));
  MI_TRY(ls_finish(part, p.grid_map, loss, Nm, loss_weight, 1, st));
  if (!want) return MI_OK;
  const float gscale = (float)(-(double)loss_weight / Nm);
  return with_dtype(dtype, "ssim_loss", [&](auto tag) -> int {
    using T = decltype(tag);
    ProfScope ps(st, K_L1, Nm * 12 + N * 3 * dtype_size(dtype), N * 100);
    hipLaunchKernelGGL((ssim_grad_kernel<T>), dim3(p.grid_grad), dim3(LS_THREADS), 0, st, (const T*)pred, (const T*)target, ga, gb,
                       gc, (T*)dpred, H, W, p.Hm, p.Wm, p.itx, p.ity, win, gscale);
    MI_LAUNCH_CHECK();
    return MI_OK;
  });
}
