// BatchNorm2d over an activation tensor and the scaled residual out = f s[c] + x: the two pieces of SFHformer's Block
// (SFHformer.py:254-282) that are neither its Mixer nor its FFN.  x, y, f, out, the cotangents [B, C, H, W] in fp32 or bf16, N = H W;
// parameters, statistics and parameter gradients fp32; all arithmetic between load and store fp32.
// A plane is cut into chunks of BN_CHUNK = 4096 elements; ONE workgroup of 256 threads owns one chunk of one plane, so the channel's
// constants are wave-uniform and no thread divides.  Thread t holds 16 elements of its chunk in registers: with V = 16 bytes /
// sizeof(T) (4 fp32, 8 bf16) its slot i is element ((i / V) 256 + t) V + i % V of the chunk - a 16-byte access per V slots where N % V
// == 0 and the pointers are 16-byte aligned, the SAME elements one by one where not (odd N with B C > 1), so which form runs never
// changes which thread sums what.
//   bn_stats_kernel    chunk -> (mean, M2 = sum of squared deviations from that mean), the chunk held in registers between the two
//                      block sums: x is read once, two large sums are never differenced
//   bn_finish_kernel   one thread per channel merges its B nchunk pairs in order (image, then chunk; Chan's update), writes
//                      stat = (mu[C], r[C]) and updates the running statistics in place
//   bn_apply_kernel    y = (x - mu) (w r) + b; eval mode: (mu, r) from the running statistics in the same launch
//   bn_bwd_sums_kernel chunk -> (sum dy, sum dy xhat);  bn_bwd_finish_kernel -> dw, db and the two means pass two subtracts
//   bn_bwd_dx_kernel   dx = w r ((dy - mean dy) - xhat mean(dy xhat)) (+ dres); eval mode: w r dy (+ dres)
//   sr_fwd_kernel      out = f s + x; with part_out also the (mean, M2) pair of its chunk of out AS STORED: chunk_stats is written
//                      once and instantiated where the chunk is loaded (bn_stats_kernel) and where it is computed and stored (here)
//   sr_bwd_kernel      df = dout s and the chunk's sum of f dout;  sr_finish_kernel -> ds
// Sums: a thread adds its 16 slots in order, the wave sums by wave_sum (a pairwise tree over adjacent lanes), the four waves as
// (w0 + w1) + (w2 + w3): a fixed order.  No atomics; bitwise reproducible.  Floating-point contraction is off in this file: every
// product and sum rounds on its own, so tests/bn2d_ref.py can state the same operations in the same order.
// Streams touched once in a call load and store through the non-temporal Vec forms of common.h; x in the statistics pass and x, dy in
// the backward's sum pass are read again by the next launch and load with the default policy.
#include "internal.h"

#pragma clang fp contract(off)

namespace mi {
namespace {

constexpr int BN_THREADS = 256, BN_SLOTS = 16, BN_CHUNK = BN_THREADS * BN_SLOTS, BN_MAX_C = 4096;
constexpr int BN_MAX_GRID = 1 << 20;             // workgroups per launch (grid x block stays below 2^32); the rest by a grid stride
template <typename T> struct Geo { static constexpr int V = 16 / (int)sizeof(T), A = BN_SLOTS / V; };

// Sum over the 256 threads in a fixed order (wave sums on the VALU, then the four of them); every thread gets the total.
__device__ __forceinline__ float block_sum(float v, float* lds) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// 16 bytes with the default cache policy (the Vec forms of common.h are non-temporal)
__device__ __forceinline__ void ld16_keep(const float* p, float* o) {
  const f32x4 t = *reinterpret_cast<const f32x4*>(p);
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
}
__device__ __forceinline__ void ld16_keep(const bf16* p, float* o) {
  const u32x4 t = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[2 * i] = bf16_bits_to_f32(t[i] & 0xffffu); o[2 * i + 1] = bf16_bits_to_f32(t[i] >> 16); }
}

// element of the chunk that slot i of this thread holds
template <typename T> __device__ __forceinline__ int slot_elem(int i) {
  constexpr int V = Geo<T>::V;
  return ((i / V) * BN_THREADS + (int)threadIdx.x) * V + i % V;
}
// This thread's slots of the chunk at p; `left` elements of the plane remain from p on; slots past the plane's end read as 0.
template <typename T, bool NT>
__device__ __forceinline__ void chunk_ld(const T* __restrict__ p, int left, int vec, float (&v)[BN_SLOTS]) {
  constexpr int V = Geo<T>::V, A = Geo<T>::A;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const int e = (j * BN_THREADS + (int)threadIdx.x) * V;
    if (vec) {                                   // N % V == 0: the V slots are inside the plane together or not at all
      if (e < left) {
        if constexpr (NT) Vec<T, V>::ld(p + e, &v[j * V]); else ld16_keep(p + e, &v[j * V]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[j * V + k] = 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) v[j * V + k] = e + k < left ? ld1(p + e + k) : 0.f;
    }
  }
}
template <typename T>
__device__ __forceinline__ void chunk_st(T* __restrict__ p, int left, int vec, const float (&v)[BN_SLOTS]) {
  constexpr int V = Geo<T>::V, A = Geo<T>::A;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const int e = (j * BN_THREADS + (int)threadIdx.x) * V;
    if (vec) {
      if (e < left) Vec<T, V>::st(p + e, &v[j * V]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (e + k < left) st1(p + e + k, v[j * V + k]);
    }
  }
}

// (mean, M2) of the chunk whose values the workgroup holds in v (0 in the slots past the plane's end) -> out2[0], out2[1]
template <typename T>
__device__ __forceinline__ void chunk_stats(const float (&v)[BN_SLOTS], int left, float* red, float* __restrict__ out2) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < BN_SLOTS; ++i) s += v[i];
  const float mean = block_sum(s, red) / (float)min(left, BN_CHUNK);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < BN_SLOTS; ++i) {
    const float d = slot_elem<T>(i) < left ? v[i] - mean : 0.f;
    q += d * d;
  }
  q = block_sum(q, red);
  if (threadIdx.x == 0) { out2[0] = mean; out2[1] = q; }
}

// Workgroup `wg` of total = B C nchunk: chunk k of plane wg / nchunk (channel plane % C).
struct ChunkId { int64_t base; int c, left; };
__device__ __forceinline__ ChunkId chunk_id(int wg, int C, int N, int nchunk) {
  const int plane = wg / nchunk, k = wg - plane * nchunk;
  return ChunkId{(int64_t)plane * N + (int64_t)k * BN_CHUNK, plane % C, N - k * BN_CHUNK};
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm forward
// part [B][C][nchunk][2]
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, int C, int N, int nchunk,
                                                              int total, int vec) {
  __shared__ float red[4];
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    float v[BN_SLOTS];
    chunk_ld<T, false>(x + id.base, id.left, vec, v);
    chunk_stats<T>(v, id.left, red, part + 2 * (int64_t)wg);
  }
}

// One thread per channel: Chan's update over the channel's B nchunk pairs, image by image and chunk by chunk.
__global__ __launch_bounds__(BN_THREADS) void bn_finish_kernel(const float* __restrict__ part, int B, int C, int N, int nchunk, float eps,
                                                               float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                               float* __restrict__ stat) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c >= C) return;
  int cnt = 0;
  float mean = 0.f, m2 = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = part + 2 * ((int64_t)b * C + c) * nchunk;
#pragma unroll 4                              // (the loads of four trips in flight; the order of the sum is unchanged)
    for (int k = 0; k < nchunk; ++k) {
      const int nb = min(N - k * BN_CHUNK, BN_CHUNK), tot = cnt + nb;
      const float d = p[2 * k] - mean, w = (float)nb / (float)tot;
      mean = mean + d * w;
      m2 = (m2 + p[2 * k + 1]) + (d * d) * ((float)cnt * w);
      cnt = tot;
    }
  }
  const float var = m2 / (float)cnt;
  stat[c] = mean;
  stat[C + c] = 1.0f / sqrtf(var + eps);
  rmean[c] = (1.0f - momentum) * rmean[c] + momentum * mean;
  rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (var * ((float)cnt / (float)(cnt - 1)));
}

// eval: (mu, r) from the running statistics (and into stat, where one is asked for, by the workgroup of image 0, chunk 0)
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                              const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                              float* __restrict__ stat, T* __restrict__ y, int C, int N, int nchunk, int total,
                                                              int eval, float eps, int vec) {
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    float mu, r;
    if (eval) {
      mu = rmean[id.c];
      r = 1.0f / sqrtf(rvar[id.c] + eps);
      if (stat && wg < C * nchunk && id.left == N && threadIdx.x == 0) { stat[id.c] = mu; stat[C + id.c] = r; }
    } else {
      mu = stat[id.c];
      r = stat[C + id.c];
    }
    const float g = w[id.c] * r, be = b[id.c];
    float v[BN_SLOTS];
    chunk_ld<T, true>(x + id.base, id.left, vec, v);
#pragma unroll
    for (int i = 0; i < BN_SLOTS; ++i) v[i] = (v[i] - mu) * g + be;
    chunk_st<T>(y + id.base, id.left, vec, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm backward
// part [B][C][nchunk][2] = (sum dy, sum dy xhat) of the chunk
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_sums_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ stat,
                                                                 float* __restrict__ part, int C, int N, int nchunk, int total, int vec) {
  __shared__ float red[4];
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    const float mu = stat[id.c], r = stat[C + id.c];
    float xv[BN_SLOTS], dv[BN_SLOTS];
    chunk_ld<T, false>(x + id.base, id.left, vec, xv);
    chunk_ld<T, false>(dy + id.base, id.left, vec, dv);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < BN_SLOTS; ++i) {         // (a slot past the plane's end holds dy = 0)
      s1 += dv[i];
      s2 += dv[i] * ((xv[i] - mu) * r);
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) { part[2 * (int64_t)wg] = s1; part[2 * (int64_t)wg + 1] = s2; }
  }
}

// One thread per channel: db = sum dy, dw = sum dy xhat over the channel's pairs in order; coef = (mean dy, mean dy xhat) in
// training mode, (0, 0) in eval mode.
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_finish_kernel(const float* __restrict__ part, int B, int C, int nchunk, float inv_n,
                                                                   int training, float* __restrict__ dw, float* __restrict__ db,
                                                                   float* __restrict__ coef, int accumulate) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = part + 2 * ((int64_t)b * C + c) * nchunk;
#pragma unroll 4                              // (the loads of four trips in flight; the order of the sum is unchanged)
    for (int k = 0; k < nchunk; ++k) { s1 += p[2 * k]; s2 += p[2 * k + 1]; }
  }
  db[c] = accumulate ? db[c] + s1 : s1;
  dw[c] = accumulate ? dw[c] + s2 : s2;
  coef[c] = training ? s1 * inv_n : 0.f;
  coef[C + c] = training ? s2 * inv_n : 0.f;
}

template <typename T, bool RES>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_dx_kernel(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ dres,
                                                               const float* __restrict__ w, const float* __restrict__ stat,
                                                               const float* __restrict__ coef, T* __restrict__ dx, int C, int N, int nchunk,
                                                               int total, int training, int vec) {
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    const float mu = stat[id.c], r = stat[C + id.c], g = w[id.c] * r, c1 = coef[id.c], c2 = coef[C + id.c];
    float v[BN_SLOTS];
    chunk_ld<T, true>(dy + id.base, id.left, vec, v);
    if (training) {                              // wave-uniform
      float xv[BN_SLOTS];
      chunk_ld<T, true>(x + id.base, id.left, vec, xv);
#pragma unroll
      for (int i = 0; i < BN_SLOTS; ++i) v[i] = g * ((v[i] - c1) - ((xv[i] - mu) * r) * c2);
    } else {
#pragma unroll
      for (int i = 0; i < BN_SLOTS; ++i) v[i] = g * v[i];
    }
    if constexpr (RES) {
      float rv[BN_SLOTS];
      chunk_ld<T, true>(dres + id.base, id.left, vec, rv);
#pragma unroll
      for (int i = 0; i < BN_SLOTS; ++i) v[i] += rv[i];
    }
    chunk_st<T>(dx + id.base, id.left, vec, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------- scaled residual
template <typename T, bool STATS>
__global__ __launch_bounds__(BN_THREADS) void sr_fwd_kernel(const T* __restrict__ f, const T* __restrict__ x, const float* __restrict__ scale,
                                                            T* __restrict__ out, float* __restrict__ part, int C, int N, int nchunk, int total,
                                                            int vec) {
  __shared__ float red[4];
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    const float s = scale[id.c];
    float v[BN_SLOTS], xv[BN_SLOTS];
    chunk_ld<T, true>(f + id.base, id.left, vec, v);
    chunk_ld<T, true>(x + id.base, id.left, vec, xv);
#pragma unroll
    for (int i = 0; i < BN_SLOTS; ++i) v[i] = to_f32(Cvt<T>::from(v[i] * s + xv[i]));   // out as stored
    chunk_st<T>(out + id.base, id.left, vec, v);
    if constexpr (STATS) chunk_stats<T>(v, id.left, red, part + 2 * (int64_t)wg);
  }
}

// part [B][C][nchunk] = the chunk's sum of f dout
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void sr_bwd_kernel(const T* __restrict__ f, const T* __restrict__ dout, const float* __restrict__ scale,
                                                            T* __restrict__ df, float* __restrict__ part, int C, int N, int nchunk, int total,
                                                            int vec) {
  __shared__ float red[4];
  for (int wg = blockIdx.x; wg < total; wg += gridDim.x) {
    const ChunkId id = chunk_id(wg, C, N, nchunk);
    const float s = scale[id.c];
    float fv[BN_SLOTS], dv[BN_SLOTS];
    chunk_ld<T, true>(f + id.base, id.left, vec, fv);
    chunk_ld<T, true>(dout + id.base, id.left, vec, dv);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < BN_SLOTS; ++i) {
      acc += fv[i] * dv[i];
      dv[i] = dv[i] * s;
    }
    chunk_st<T>(df + id.base, id.left, vec, dv);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[wg] = acc;
  }
}

__global__ __launch_bounds__(BN_THREADS) void sr_finish_kernel(const float* __restrict__ part, int B, int C, int nchunk, float* __restrict__ ds,
                                                               int accumulate) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = part + ((int64_t)b * C + c) * nchunk;
#pragma unroll 4                              // (the loads of four trips in flight; the order of the sum is unchanged)
    for (int k = 0; k < nchunk; ++k) s += p[k];
  }
  ds[c] = accumulate ? ds[c] + s : s;
}

// ---------------------------------------------------------------------------------------------------------------- the plan
enum { BS_PART = 0, BS_STAT, BS_COEF, BS_SECTIONS };
struct BnPlan {
  int B, C, H, W, dtype, training, N;
  float eps, momentum;
  int nchunk, parts, width;                      // chunks per plane; partials per channel (B nchunk); elements per access the shape allows
  int total, grid, grid_chan;                    // B C nchunk workgroups of work; the per-chunk launches' grid; the finish kernels' grid
  int fwd, fwd_part_in, bwd;                     // launches
  Sections<BS_SECTIONS> ws;
  size_t stat_bytes;
};

// bn: BatchNorm's own checks (eps, momentum, the count) and sections; else the scaled residual's (the three fields are not read)
int bn_check(const char* who, const mi_bn2d_shape* s, bool bn, BnPlan* p) {
  MI_CHECK_ARG(s, "%s: null shape", who);
  const int B = s->B, Cn = s->C, H = s->H, W = s->W, dt = s->dtype;
  MI_CHECK_ARG(dt == MI_F32 || dt == MI_BF16, "%s: bad dtype %d", who, dt);
  MI_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d (each at least 1)", who, B, H, W);
  MI_CHECK_ARG(Cn >= 1 && Cn <= BN_MAX_C, "%s: C=%d outside the supported 1..%d", who, Cn, BN_MAX_C);
  const double elems = (double)B * Cn * (double)H * (double)W;
  MI_CHECK_ARG(elems < 2147483648.0, "%s: B*C*H*W = %.0f elements, beyond the 2^31 the kernels index", who, elems);
  memset(p, 0, sizeof(*p));
  p->B = B; p->C = Cn; p->H = H; p->W = W; p->dtype = dt; p->N = H * W;
  if (bn) {
    MI_CHECK_ARG(s->eps > 0.f, "%s: eps=%g must be positive", who, (double)s->eps);
    MI_CHECK_ARG(s->momentum >= 0.f && s->momentum <= 1.f, "%s: momentum=%g outside 0..1", who, (double)s->momentum);
    p->training = s->training ? 1 : 0;
    MI_CHECK_ARG(!p->training || (int64_t)B * p->N > 1, "%s: training needs more than 1 value per channel (B*H*W = 1)", who);
    p->eps = s->eps; p->momentum = s->momentum;
  }
  p->nchunk = cdiv(p->N, BN_CHUNK);
  p->parts = B * p->nchunk;
  p->width = p->N % (16 / (int)dtype_size(dt)) == 0 ? 16 / (int)dtype_size(dt) : 1;
  p->total = B * Cn * p->nchunk;
  p->grid = p->total < BN_MAX_GRID ? p->total : BN_MAX_GRID;
  p->grid_chan = cdiv(Cn, BN_THREADS);
  Sections<BS_SECTIONS>& ws = p->ws;
  if (bn) {
    p->fwd = p->training ? 3 : 1; p->fwd_part_in = p->training ? 2 : 1; p->bwd = 3;
    ws.put(BS_PART, (size_t)p->total * 2 * sizeof(float));      // forward: (mean, M2); backward: (sum dy, sum dy xhat)
    ws.put(BS_STAT, (size_t)2 * Cn * sizeof(float));            // (mu, r) of a forward that is given no stat
    ws.put(BS_COEF, (size_t)2 * Cn * sizeof(float));            // backward: (mean dy, mean dy xhat)
  } else {
    p->fwd = 1; p->fwd_part_in = 1; p->bwd = 2;
    ws.put(BS_PART, (size_t)p->total * sizeof(float));          // backward: the chunks' sums of f dout
    ws.put(BS_STAT, 0); ws.put(BS_COEF, 0);
  }
  p->stat_bytes = (size_t)2 * Cn * sizeof(float);
  return MI_OK;
}

// 16 scalars, the BS_* sections from [16]; tail: workspace, stat and forward-partial bytes (the format: plan_report, internal.h)
int bn_plan_out(const BnPlan& p, int64_t* out) {
  return plan_report<16>(out, {p.B, p.C, p.N, p.dtype, p.training, BN_THREADS, BN_CHUNK, p.nchunk, p.parts, p.width, p.total, p.grid,
                               p.grid_chan, p.fwd, p.fwd_part_in, p.bwd},
                         p.ws, {(int64_t)p.ws.total, (int64_t)p.stat_bytes, (int64_t)p.total * 2 * (int64_t)sizeof(float)});
}

int bn_vec(const BnPlan& p, std::initializer_list<const void*> ptrs) {
  if (p.width == 1) return 0;
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return 0;
  return 1;
}

}  // namespace
}  // namespace mi

using namespace mi;

// ---------------------------------------------------------------------------------------------------------------- BatchNorm2d
extern "C" size_t mi_bn2d_workspace(const mi_bn2d_shape* s) {
  BnPlan p;
  return bn_check("bn2d_workspace", s, true, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" int mi_bn2d_plan(const mi_bn2d_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "bn2d_plan: null pointer");
  BnPlan p;
  MI_TRY(bn_check("bn2d_plan", s, true, &p));
  return bn_plan_out(p, out);
}

extern "C" int mi_bn2d_fwd(const mi_bn2d_shape* s, const float* w, const float* b, const void* x, void* y, float* running_mean,
                           float* running_var, float* stat, const float* part_in, void* ws, void* stream) {
  BnPlan p;
  MI_TRY(bn_check("bn2d_fwd", s, true, &p));
  MI_CHECK_ARG(w && b && x && y && running_mean && running_var && ws, "bn2d_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int vec = bn_vec(p, {x, y});
  float* part = p.ws.at(ws, BS_PART);
  float* stat_use = stat ? stat : p.ws.at(ws, BS_STAT);
  return with_dtype(p.dtype, "bn2d_fwd", [&](auto tag) -> int {
    using T = decltype(tag);
    if (p.training) {
      if (!part_in) {
        hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)x, part, p.C, p.N, p.nchunk, p.total, vec);
        MI_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(bn_finish_kernel, dim3(p.grid_chan), dim3(BN_THREADS), 0, st, part_in ? part_in : (const float*)part, p.B, p.C, p.N,
                         p.nchunk, p.eps, p.momentum, running_mean, running_var, stat_use);
      MI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)x, w, b, (const float*)running_mean,
                       (const float*)running_var, p.training ? stat_use : stat, (T*)y, p.C, p.N, p.nchunk, p.total, p.training ? 0 : 1, p.eps,
                       vec);
    MI_LAUNCH_CHECK();
    return MI_OK;
  });
}

extern "C" int mi_bn2d_bwd(const mi_bn2d_shape* s, const float* w, const void* x, const void* dy, const void* dres, void* dx, float* dw,
                           float* db, int accumulate, const float* stat, void* ws, void* stream) {
  BnPlan p;
  MI_TRY(bn_check("bn2d_bwd", s, true, &p));
  MI_CHECK_ARG(w && x && dy && dx && stat && ws, "bn2d_bwd: null pointer");
  MI_CHECK_ARG(dw && db, "bn2d_bwd: null gradient buffer");
  hipStream_t st = (hipStream_t)stream;
  const int vec = bn_vec(p, {x, dy, dres, dx});
  float* part = p.ws.at(ws, BS_PART);
  float* coef = p.ws.at(ws, BS_COEF);
  const float inv_n = 1.0f / (float)((int64_t)p.B * p.N);
  return with_dtype(p.dtype, "bn2d_bwd", [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn_bwd_sums_kernel<T>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)x, (const T*)dy, stat, part, p.C, p.N, p.nchunk,
                       p.total, vec);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(p.grid_chan), dim3(BN_THREADS), 0, st, (const float*)part, p.B, p.C, p.nchunk, inv_n,
                       p.training, dw, db, coef, accumulate ? 1 : 0);
    MI_LAUNCH_CHECK();
    if (dres)
      hipLaunchKernelGGL((bn_bwd_dx_kernel<T, true>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)x, (const T*)dy, (const T*)dres, w, stat,
                         (const float*)coef, (T*)dx, p.C, p.N, p.nchunk, p.total, p.training, vec);
    else
      hipLaunchKernelGGL((bn_bwd_dx_kernel<T, false>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)x, (const T*)dy, (const T*)nullptr, w,
                         stat, (const float*)coef, (T*)dx, p.C, p.N, p.nchunk, p.total, p.training, vec);
    MI_LAUNCH_CHECK();
    return MI_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------- scaled residual
extern "C" size_t mi_scale_res_workspace(const mi_scale_res_shape* s) {
  BnPlan p;
  return bn_check("scale_res_workspace", s, false, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" int mi_scale_res_plan(const mi_scale_res_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "scale_res_plan: null pointer");
  BnPlan p;
  MI_TRY(bn_check("scale_res_plan", s, false, &p));
  return bn_plan_out(p, out);
}

extern "C" int mi_scale_res_fwd(const mi_scale_res_shape* s, const float* scale, const void* f, const void* x, void* out, float* part_out,
                                void* stream) {
  BnPlan p;
  MI_TRY(bn_check("scale_res_fwd", s, false, &p));
  MI_CHECK_ARG(scale && f && x && out, "scale_res_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int vec = bn_vec(p, {f, x, out});
  return with_dtype(p.dtype, "scale_res_fwd", [&](auto tag) {
    using T = decltype(tag);
    if (part_out)
      hipLaunchKernelGGL((sr_fwd_kernel<T, true>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)f, (const T*)x, scale, (T*)out, part_out, p.C,
                         p.N, p.nchunk, p.total, vec);
    else
      hipLaunchKernelGGL((sr_fwd_kernel<T, false>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)f, (const T*)x, scale, (T*)out,
                         (float*)nullptr, p.C, p.N, p.nchunk, p.total, vec);
  });
}

extern "C" int mi_scale_res_bwd(const mi_scale_res_shape* s, const float* scale, const void* f, const void* dout, void* df, float* dscale,
                                int accumulate, void* ws, void* stream) {
  BnPlan p;
  MI_TRY(bn_check("scale_res_bwd", s, false, &p));
  MI_CHECK_ARG(scale && f && dout && df && ws, "scale_res_bwd: null pointer");
  MI_CHECK_ARG(dscale, "scale_res_bwd: null gradient buffer");
  hipStream_t st = (hipStream_t)stream;
  float* part = p.ws.at(ws, BS_PART);
  const int vec = bn_vec(p, {f, dout, df});
  return with_dtype(p.dtype, "scale_res_bwd", [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((sr_bwd_kernel<T>), dim3(p.grid), dim3(BN_THREADS), 0, st, (const T*)f, (const T*)dout, scale, (T*)df, part, p.C, p.N,
                       p.nchunk, p.total, vec);
    MI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sr_finish_kernel, dim3(p.grid_chan), dim3(BN_THREADS), 0, st, (const float*)part, p.B, p.C, p.nchunk, dscale,
                       accumulate ? 1 : 0);
    MI_LAUNCH_CHECK();
    return MI_OK;
  });
}
