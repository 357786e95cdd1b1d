// SFHformer's TokenMixer_For_Gloal (SFHformer.py:183-206) and Mixer (:209-251): the kernels that neither the 1x1 product, the
// FourierUnit nor the local mixer cover, and the two launch sequences that tie those library calls together.
//   Gloal(b)  u1 = Wi b + bi;  p = gelu(u1);  f = FourierUnit(p);  r = f + p;  u2 = Wf r + bf;  q = gelu(u2)
//   Mixer(x)  [a; b] = conv_init(x);  l = Local(a);  g = gelu(cat(l, q))  (the global half passes GELU twice);
//             m = mean_N g;  s = sigmoid(W2 relu(W1 m + b1) + b2);  out = (Wc diag(s_b)) g + bc
// Own kernels (fp32 arithmetic on fp32 / bf16 planes, 16-byte accesses where N % 4 == 0 and the pointers allow it, else element
// by element; no atomics, every sum in a fixed order: bitwise reproducible):
//   sm_ew_kernel     flat passes: p = gelu(u1) / q = gelu(u2);  r = f + p;  du2 = dq gelu'(u2);  du1 = (dr + dp) gelu'(u1)
//   sm_tail_in       reads l and u2 once, writes g into ONE [B, 2dim, N] tensor (that tensor is the cat) and, per (image, channel),
//                    `pool` partial sums of g as stored
//   sm_ca_kernel     one workgroup per image: partials -> m -> hidden -> s in fp32, and the folded weight Wc diag(s_b) [dim, 2dim]
//   sm_gate_bwd      one workgroup per image, from the per-image Gram P_b = dout_b g_b^T: ds = sum_m Wc . P_b, then the gate's
//                    backward down to dm / N
//   sm_gate_wgrad    dWc = sum_b P_b diag(s_b), dW1, db1, dW2, db2: one thread per element, the images in order
//   sm_tail_back     dl = (e + dm/N) gelu'(l);  du2 = (e + dm/N) gelu'(q) gelu'(u2), q = gelu(u2) recomputed
// s g is never written: ca_conv is one mi_pw_gemm with a per-image weight, its transposed form gives e = (Wc diag(s_b))^T dout.
// GELU as in sfh_ffn.hip: libm erfc / exp in the fp32 instantiation, gelu_parts in bf16.
#include "internal.h"

namespace mi {
namespace {

constexpr int SM_THREADS = 256, SM_MAX_POOL = 16, SM_POOL_ELEMS = 4096, SM_MAX_DIM = 128, SM_MIN_HW = 2, SM_MAX_HW = 512;
enum { SM_GLOBAL = 0, SM_MIXER = 1 };
enum { EW_GELU = 0, EW_ADD, EW_DGELU, EW_ADD_DGELU };

template <typename T> __device__ __forceinline__ void sm_gelu_parts(float x, float& cdf, float& pdf) { gelu_parts(x, cdf, pdf); }
template <> __device__ __forceinline__ void sm_gelu_parts<float>(float x, float& cdf, float& pdf) {
  cdf = 0.5f * erfcf(-0.70710678118654752440f * x);
  pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
}
template <typename T> __device__ __forceinline__ float sm_stored(float v) { return to_f32(Cvt<T>::from(v)); }

// ------------------------------------------------------------------ flat elementwise passes
template <typename T, int MODE>
__device__ __forceinline__ float sm_ew(float a, float b, float u) {
  if constexpr (MODE == EW_ADD) return a + b;
  float cdf, pdf;
  sm_gelu_parts<T>(MODE == EW_GELU ? a : u, cdf, pdf);
  if constexpr (MODE == EW_GELU) return a * cdf;
  if constexpr (MODE == EW_DGELU) return a * (cdf + u * pdf);
  return (a + b) * (cdf + u * pdf);
}
// y[i] = f(a[i], b[i], u[i]) over n elements; vec: n % 4 == 0 and every pointer 16-byte aligned.  y may be a or b (same index).
template <typename T, int MODE>
__global__ __launch_bounds__(SM_THREADS) void sm_ew_kernel(const T* a, const T* b, const T* u, T* y, int64_t n, int vec) {
  const int64_t step = (int64_t)gridDim.x * SM_THREADS, t0 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (vec) {
    for (int64_t i = t0; i < n / 4; i += step) {
      float av[4], bv[4] = {0.f, 0.f, 0.f, 0.f}, uv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4];
      Vec<T, 4>::ld(a + 4 * i, av);
      if constexpr (MODE == EW_ADD || MODE == EW_ADD_DGELU) Vec<T, 4>::ld(b + 4 * i, bv);
      if constexpr (MODE == EW_DGELU || MODE == EW_ADD_DGELU) Vec<T, 4>::ld(u + 4 * i, uv);
#pragma unroll
      for (int k = 0; k < 4; ++k) yv[k] = sm_ew<T, MODE>(av[k], bv[k], uv[k]);
      Vec<T, 4>::st(y + 4 * i, yv);
    }
  } else {
    for (int64_t i = t0; i < n; i += step) {
      const float av = ld1(a + i);
      float bv = 0.f, uv = 0.f;
      if constexpr (MODE == EW_ADD || MODE == EW_ADD_DGELU) bv = ld1(b + i);
      if constexpr (MODE == EW_DGELU || MODE == EW_ADD_DGELU) uv = ld1(u + i);
      st1(y + i, sm_ew<T, MODE>(av, bv, uv));
    }
  }
}

// ------------------------------------------------------------------ the tail, forward
// grid (pool, 2dim, B).  Channel ch < dim: g = gelu(l); else g = gelu(gelu(u2)).  Workgroup `split` of a plane walks every pool-th
// block of 1024 elements; part[(b 2dim + ch) pool + split] = the sum of its g values as stored.
template <typename T>
__global__ __launch_bounds__(SM_THREADS) void sm_tail_in(const T* __restrict__ l, const T* __restrict__ u2, T* __restrict__ g,
                                                         float* __restrict__ part, int dim, int64_t N, int vec) {
  __shared__ float red[4];
  const int ch = blockIdx.y, b = blockIdx.z, C2 = 2 * dim, split = blockIdx.x, pool = gridDim.x;
  const bool glo = ch >= dim;
  const T* src = glo ? u2 + ((int64_t)b * dim + (ch - dim)) * N : l + ((int64_t)b * dim + ch) * N;
  T* dst = g + ((int64_t)b * C2 + ch) * N;
  float acc[1] = {0.f};
  auto one = [&](float v) {
    float cdf, pdf;
    sm_gelu_parts<T>(v, cdf, pdf);
    v *= cdf;
    if (glo) {
      sm_gelu_parts<T>(v, cdf, pdf);
      v *= cdf;
    }
    return sm_stored<T>(v);
  };
  if (vec) {
    for (int64_t i = (int64_t)split * SM_THREADS + threadIdx.x; i < N / 4; i += (int64_t)pool * SM_THREADS) {
      float v[4];
      Vec<T, 4>::ld(src + 4 * i, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = one(v[k]);
      acc[0] += (v[0] + v[1]) + (v[2] + v[3]);
      Vec<T, 4>::st(dst + 4 * i, v);
    }
  } else {
    for (int64_t i = (int64_t)split * SM_THREADS + threadIdx.x; i < N; i += (int64_t)pool * SM_THREADS) {
      const float v = one(ld1(src + i));
      acc[0] += v;
      st1(dst + i, v);
    }
  }
  const float tot = block_sum4<1>(acc, red);
  if (threadIdx.x == 0) part[((int64_t)b * C2 + ch) * pool + split] = tot;
}

// grid (B).  m, s [B, 2dim], hid [B, dim] (after the ReLU), fold [B, dim, 2dim] = Wc diag(s_b).
__global__ __launch_bounds__(SM_THREADS) void sm_ca_kernel(const float* __restrict__ part, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ wc,
                                                           float* __restrict__ m, float* __restrict__ hid, float* __restrict__ s,
                                                           float* __restrict__ fold, int dim, int pool, float inv_n) {
  __shared__ float sm[2 * SM_MAX_DIM], sh[SM_MAX_DIM], ss[2 * SM_MAX_DIM];
  const int b = blockIdx.x, C2 = 2 * dim, t = threadIdx.x;
  if (t < C2) {
    const float* p = part + ((int64_t)b * C2 + t) * pool;
    float acc = 0.f;
    for (int i = 0; i < pool; ++i) acc += p[i];
    sm[t] = acc * inv_n;
    m[(int64_t)b * C2 + t] = sm[t];
  }
  __syncthreads();
  if (t < dim) {
    float acc = b1[t];
    for (int c = 0; c < C2; ++c) acc = fmaf(w1[t * C2 + c], sm[c], acc);
    sh[t] = fmaxf(acc, 0.f);
    hid[(int64_t)b * dim + t] = sh[t];
  }
  __syncthreads();
  if (t < C2) {
    float acc = b2[t];
    for (int j = 0; j < dim; ++j) acc = fmaf(w2[t * dim + j], sh[j], acc);
    ss[t] = 1.0f / (1.0f + expf(-acc));
    s[(int64_t)b * C2 + t] = ss[t];
  }
  __syncthreads();
  float* f = fold + (int64_t)b * dim * C2;
  for (int i = t; i < dim * C2; i += SM_THREADS) f[i] = wc[i] * ss[i % C2];
}

// ------------------------------------------------------------------ the tail, backward
// grid (B).  P [B, dim, 2dim] = dout_b g_b^T.  dz2 [B, 2dim], dz1 [B, dim], dmn [B, 2dim] = dm / N.
__global__ __launch_bounds__(SM_THREADS) void sm_gate_bwd(const float* __restrict__ P, const float* __restrict__ wc, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, const float* __restrict__ hid, const float* __restrict__ s,
                                                          float* __restrict__ dz2, float* __restrict__ dz1, float* __restrict__ dmn, int dim,
                                                          float inv_n) {
  __shared__ float z2[2 * SM_MAX_DIM], z1[SM_MAX_DIM];
  const int b = blockIdx.x, C2 = 2 * dim, t = threadIdx.x;
  if (t < C2) {
    const float* Pb = P + (int64_t)b * dim * C2;
    float ds = 0.f;
    for (int r = 0; r < dim; ++r) ds = fmaf(wc[r * C2 + t], Pb[r * C2 + t], ds);
    const float sv = s[(int64_t)b * C2 + t];
    z2[t] = ds * sv * (1.0f - sv);
    dz2[(int64_t)b * C2 + t] = z2[t];
  }
  __syncthreads();
  if (t < dim) {
    float dh = 0.f;
    for (int c = 0; c < C2; ++c) dh = fmaf(w2[c * dim + t], z2[c], dh);
    z1[t] = hid[(int64_t)b * dim + t] > 0.f ? dh : 0.f;
    dz1[(int64_t)b * dim + t] = z1[t];
  }
  __syncthreads();
  if (t < C2) {
    float dm = 0.f;
    for (int j = 0; j < dim; ++j) dm = fmaf(w1[j * C2 + t], z1[j], dm);
    dmn[(int64_t)b * C2 + t] = dm * inv_n;
  }
}

// One thread per gradient element, the images summed in order.  Elements: dWc [dim, 2dim], dW2 [2dim, dim], dW1 [dim, 2dim],
// db2 [2dim], db1 [dim].
__global__ __launch_bounds__(SM_THREADS) void sm_gate_wgrad(const float* __restrict__ P, const float* __restrict__ m, const float* __restrict__ hid,
                                                            const float* __restrict__ s, const float* __restrict__ dz2, const float* __restrict__ dz1,
                                                            float* __restrict__ gwc, float* __restrict__ gw1, float* __restrict__ gb1,
                                                            float* __restrict__ gw2, float* __restrict__ gb2, int B, int dim, int accumulate) {
  const int C2 = 2 * dim, mat = dim * C2, total = 3 * mat + C2 + dim;
  const int i = blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= total) return;
  float acc = 0.f;
  float* out;
  if (i < mat) {                                             // dWc[r, c] = sum_b P_b[r, c] s_b[c]
    const int c = i % C2;
    for (int b = 0; b < B; ++b) acc = fmaf(P[(int64_t)b * mat + i], s[(int64_t)b * C2 + c], acc);
    out = gwc + i;
  } else if (i < 2 * mat) {                                  // dW2[c, j] = sum_b dz2[b, c] hid[b, j]
    const int e = i - mat, c = e / dim, j = e - c * dim;
    for (int b = 0; b < B; ++b) acc = fmaf(dz2[(int64_t)b * C2 + c], hid[(int64_t)b * dim + j], acc);
    out = gw2 + e;
  } else if (i < 3 * mat) {                                  // dW1[j, c] = sum_b dz1[b, j] m[b, c]
    const int e = i - 2 * mat, j = e / C2, c = e - j * C2;
    for (int b = 0; b < B; ++b) acc = fmaf(dz1[(int64_t)b * dim + j], m[(int64_t)b * C2 + c], acc);
    out = gw1 + e;
  } else if (i < 3 * mat + C2) {
    const int c = i - 3 * mat;
    for (int b = 0; b < B; ++b) acc += dz2[(int64_t)b * C2 + c];
    out = gb2 + c;
  } else {
    const int j = i - 3 * mat - C2;
    for (int b = 0; b < B; ++b) acc += dz1[(int64_t)b * dim + j];
    out = gb1 + j;
  }
  *out = accumulate ? *out + acc : acc;
}

// grid (blocks, 2dim, B).  e [B, 2dim, N]; ch < dim: dl = (e + dmn) gelu'(l); else du2 = (e + dmn) gelu'(q) gelu'(u2), q = gelu(u2).
template <typename T>
__global__ __launch_bounds__(SM_THREADS) void sm_tail_back(const T* __restrict__ e, const T* __restrict__ l, const T* __restrict__ u2,
                                                           const float* __restrict__ dmn, T* __restrict__ dl, T* __restrict__ du2, int dim,
                                                           int64_t N, int vec) {
  const int ch = blockIdx.y, b = blockIdx.z, C2 = 2 * dim;
  const bool glo = ch >= dim;
  const int64_t po = ((int64_t)b * dim + (glo ? ch - dim : ch)) * N;
  const T* ep = e + ((int64_t)b * C2 + ch) * N;
  const T* src = (glo ? u2 : l) + po;
  T* dst = (glo ? du2 : dl) + po;
  const float add = dmn[(int64_t)b * C2 + ch];
  auto one = [&](float ev, float v) {
    float cdf, pdf;
    sm_gelu_parts<T>(v, cdf, pdf);
    float d = (ev + add);
    if (glo) {
      const float q = v * cdf;
      float cq, pq;
      sm_gelu_parts<T>(q, cq, pq);
      d *= cq + q * pq;
    }
    return d * (cdf + v * pdf);
  };
  const int64_t step = (int64_t)gridDim.x * SM_THREADS, t0 = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (vec) {
    for (int64_t i = t0; i < N / 4; i += step) {
      float ev[4], v[4];
      Vec<T, 4>::ld(ep + 4 * i, ev);
      Vec<T, 4>::ld(src + 4 * i, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = one(ev[k], v[k]);
      Vec<T, 4>::st(dst + 4 * i, v);
    }
  } else {
    for (int64_t i = t0; i < N; i += step) st1(dst + i, one(ld1(ep + i), ld1(src + i)));
  }
}

// ------------------------------------------------------------------ the plan: the ONE place that decides sections and launches
enum { MS_PW = 0, MS_GRAM, MS_CS, MS_FU, MS_LOCAL, MS_P, MS_F, MS_G, MS_SMALL, MS_FOLD, MS_PGRAM, MS_PART, MS_SCRATCH, MS_SECTIONS };
enum { SV_A = 0, SV_B, SV_L, SV_U1, SV_R, SV_U2, SV_FU, SV_SECTIONS };
enum { BW_E = 0, BW_DL, BW_DU2, BW_DA, BW_DB, BW_SECTIONS };
enum { SMALL_M = 0, SMALL_HID, SMALL_S, SMALL_DZ2, SMALL_DZ1, SMALL_DMN, SMALL_COUNT };
struct SmPlan {
  int mode, B, dim, C2, H, W, dtype;
  int64_t N, elems1, elems2;                     // elements of a [B, dim, N] / [B, 2dim, N] plane set
  int pool, ew_grid1, ew_grid2, tail_grid;       // partial sums per plane; grids of the flat passes and of the tail-back pass
  int kernels_fwd, kernels_bwd, lib_fwd, lib_bwd;
  mi_fourier_unit_shape fu;
  mi_sfh_local_shape loc;
  Sections<MS_SECTIONS> ws;
  Sections<SV_SECTIONS> saved;
  Sections<BW_SECTIONS> bw;                      // the backward's planes, overlaid on the inference copy of the saved planes
  size_t small_off[SMALL_COUNT];                 // float offsets inside MS_SMALL
};

// Mixer.conv_init (:240-241) as ONE grouped product whose two groups read the same x (x1_gs = 0) and write a and b as two dense
// [B, dim, N] tensors `gap` elements apart: mi_pw_plan gives it the instance it gives a product of one half (same family, tile
// rows and K chunks at all three levels of the network, either dtype) over twice the grid z, so it is the two products in one
// launch and one weight pack (test_sfh_mixer_cabi.py holds the two plans against each other).  No slice copy.
mi_pw_desc init_desc(const void* x, const float* w, const float* bias, void* a, int64_t gap, int dim, int B, int64_t N, int dt) {
  mi_pw_desc d = conv1x1(x, dim, w, false, dim, bias, nullptr, a, dim, B, N, dt);
  d.groups = 2; d.x1_gs = 0; d.w_gs = (int64_t)dim * dim; d.bias_gs = dim; d.y_gs = gap;
  return d;
}

template <typename S>
int sm_check(const char* who, int mode, const S* s, SmPlan* p) {
  MI_CHECK_ARG(s, "%s: null shape", who);
  const int B = s->B, dim = s->dim, H = s->H, W = s->W, dt = s->dtype;
  MI_CHECK_ARG(dt == MI_F32 || dt == MI_BF16, "%s: bad dtype %d", who, dt);
  MI_CHECK_ARG(B >= 1 && B <= 65535, "%s: bad shape B=%d (1..65535)", who, B);
  if (mode == SM_MIXER) {
    MI_CHECK_ARG(dim >= 2 && dim <= SM_MAX_DIM, "%s: dim=%d outside the supported 2..%d", who, dim, SM_MAX_DIM);
    MI_CHECK_ARG(dim % 2 == 0, "%s: dim=%d is odd: not covered (the local mixer's chunk count changes)", who, dim);
  } else {
    MI_CHECK_ARG(dim >= 1 && dim <= SM_MAX_DIM, "%s: dim=%d outside the supported 1..%d", who, dim, SM_MAX_DIM);
  }
  MI_CHECK_ARG(H >= SM_MIN_HW && H <= SM_MAX_HW, "%s: H=%d outside the supported %d..%d", who, H, SM_MIN_HW, SM_MAX_HW);
  MI_CHECK_ARG(W >= SM_MIN_HW && W <= SM_MAX_HW, "%s: W=%d outside the supported %d..%d", who, W, SM_MIN_HW, SM_MAX_HW);
  memset(p, 0, sizeof(*p));
  p->mode = mode; p->B = B; p->dim = dim; p->C2 = 2 * dim; p->H = H; p->W = W; p->dtype = dt;
  p->N = (int64_t)H * W;
  const double elems = (double)B * p->C2 * (double)p->N;
  MI_CHECK_ARG(elems < 2147483648.0, "%s: B*%d*H*W = %.0f elements, beyond the 2^31 the 1x1 path indexes", who, p->C2, elems);
  p->elems1 = (int64_t)B * dim * p->N; p->elems2 = 2 * p->elems1;
  p->fu = mi_fourier_unit_shape{B, p->C2, 4, H, W, dt, s->training ? 1 : 0, s->eps, s->momentum};
  p->loc = mi_sfh_local_shape{B, dim, H, W, dt};
  const size_t fu_ws = mi_fourier_unit_workspace(&p->fu), fu_saved = mi_fourier_unit_saved_bytes(&p->fu);
  if (!fu_ws) return MI_ERR_ARG;                             // (its own message stands: eps, momentum, the spectrum's size)
  p->pool = cdiv_cap(p->N, SM_POOL_ELEMS, SM_MAX_POOL);
  p->ew_grid1 = cdiv_cap(p->elems1, 4 * SM_THREADS, 4096);
  p->ew_grid2 = cdiv_cap(p->elems2, 4 * SM_THREADS, 4096);
  p->tail_grid = cdiv_cap(p->N, 4 * SM_THREADS, 64);

  const int C2 = p->C2;
  const int64_t N = p->N;
  const bool mix = mode == SM_MIXER;
  const size_t pl1 = (size_t)p->elems1 * dtype_size(dt), pl2 = 2 * pl1;
  Sections<SV_SECTIONS>& sv = p->saved;
  sv.put(SV_A, mix ? pl1 : 0); sv.put(SV_B, mix ? pl1 : 0); sv.put(SV_L, mix ? pl1 : 0);
  sv.put(SV_U1, pl2); sv.put(SV_R, pl2); sv.put(SV_U2, pl1); sv.put(SV_FU, fu_saved);
  Sections<BW_SECTIONS>& bw = p->bw;
  bw.put(BW_E, mix ? pl2 : 0); bw.put(BW_DL, mix ? pl1 : 0); bw.put(BW_DU2, pl1);
  bw.put(BW_DA, mix ? pl1 : 0); bw.put(BW_DB, mix ? pl1 : 0);

  Sections<MS_SECTIONS>& ws = p->ws;
  mi_pw_desc ca = per_image(probe1x1(C2, dim, false, B, N, dt)), cat = per_image(probe1x1(dim, C2, true, B, N, dt));
  mi_pw_desc dx2 = probe1x1(dim, dim, true, B, N, dt);
  dx2.x2 = PROBE_PTR; dx2.x2_bs = dx2.x1_bs; dx2.k2 = dim;
  ws.put(MS_PW, max_of({pw_ws_bytes(probe1x1(dim, C2, false, B, N, dt)), pw_ws_bytes(probe1x1(C2, dim, false, B, N, dt)),
                     pw_ws_bytes(probe1x1(dim, C2, true, B, N, dt)), pw_ws_bytes(probe1x1(C2, dim, true, B, N, dt)),
                     mix ? pw_ws_bytes(init_desc(PROBE_PTR, (const float*)PROBE_PTR, (const float*)PROBE_PTR, PROBE_PTR,
                                                 (int64_t)((sv.off[SV_B] - sv.off[SV_A]) / dtype_size(dt)), dim, B, N, dt)) : 0,
                     mix ? pw_ws_bytes(ca) : 0, mix ? pw_ws_bytes(cat) : 0,
                     mix ? pw_ws_bytes(dx2) : 0}));
  ws.put(MS_GRAM, max_of({gram_ws_bytes(probe_wgrad(dim, C2, B, N, dt)), gram_ws_bytes(probe_wgrad(C2, dim, B, N, dt)),
                       mix ? gram_ws_bytes(probe_wgrad(dim, dim, B, N, dt)) : 0, mix ? gram_ws_bytes(probe_wgrad(dim, C2, B, N, dt, 0)) : 0}));
  ws.put(MS_CS, chan_sum_workspace(C2, N));
  ws.put(MS_FU, fu_ws);
  ws.put(MS_LOCAL, mix ? mi_sfh_local_workspace(&p->loc) : 0);
  ws.put(MS_P, pl2);                                            // p; backward: the FourierUnit's input gradient
  ws.put(MS_F, pl2);                                            // f; backward: dr, then du1 in place
  ws.put(MS_G, mix ? pl2 : 0);
  size_t so = 0;
  const size_t small_n[SMALL_COUNT] = {(size_t)B * C2, (size_t)B * dim, (size_t)B * C2, (size_t)B * C2, (size_t)B * dim, (size_t)B * C2};
  for (int i = 0; i < SMALL_COUNT; ++i) { p->small_off[i] = so; so += align_up(small_n[i], 64); }
  ws.put(MS_SMALL, mix ? so * sizeof(float) : 0);
  ws.put(MS_FOLD, mix ? (size_t)B * dim * C2 * sizeof(float) : 0);
  ws.put(MS_PGRAM, mix ? (size_t)B * dim * C2 * sizeof(float) : 0);
  ws.put(MS_PART, mix ? (size_t)B * C2 * p->pool * sizeof(float) : 0);
  // forward without a blob: the saved planes (the FourierUnit's blob is never written then); backward: e, dl, du2, da, db
  ws.put(MS_SCRATCH, max_of({sv.off[SV_FU], bw.total}));
  if (mix) { p->kernels_fwd = 4; p->kernels_bwd = 6; p->lib_fwd = 6; p->lib_bwd = 12; }
  else { p->kernels_fwd = 3; p->kernels_bwd = 2; p->lib_fwd = 3; p->lib_bwd = 3; }
  return MI_OK;
}

// 15 scalars (mode, B, dim, 2dim, N, pool, three grids, threads, launch counts, the backward overlay's bytes), the MS_* sections
// from [16], the SV_* sections of the saved blob from [44] (the format: plan_report, internal.h)
int sm_plan_out(const SmPlan& p, int64_t* out) {
  return plan_report<16, 44>(out, {p.mode, p.B, p.dim, p.C2, p.N, p.pool, p.ew_grid1, p.ew_grid2, p.tail_grid, SM_THREADS, p.kernels_fwd,
                                   p.kernels_bwd, p.lib_fwd, p.lib_bwd, (int64_t)p.bw.total},
                             p.ws, p.saved, {(int64_t)p.ws.total, (int64_t)p.saved.total, 0});
}

struct GloParams { const float* init_w; const float* init_b; const float* fina_w; const float* fina_b; mi_fourier_unit_params fu; };
struct GloGrads { float* init_w; float* init_b; float* fina_w; float* fina_b; mi_fourier_unit_grads fu; };
struct Saved { void* a; void* b; void* l; void* u1; void* r; void* u2; void* fu; };
Saved sm_saved(const SmPlan& p, void* base) {
  const Sections<SV_SECTIONS>& s = p.saved;
  return Saved{s.at(base, SV_A), s.at(base, SV_B), s.at(base, SV_L), s.at(base, SV_U1),
               s.at(base, SV_R), s.at(base, SV_U2), s.at(base, SV_FU)};
}

bool sm_vec(int64_t n, std::initializer_list<const void*> ptrs) {
  if (n % 4) return false;
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return false;
  return true;
}

template <int MODE>
int sm_ew_launch(const SmPlan& p, const void* a, const void* b, const void* u, void* y, int64_t n, int grid, hipStream_t st) {
  // rows are 4 wide only where N % 4 == 0, the condition every other pass of the module uses
  const int vec = sm_vec(p.N, {a, b, u, y});
  return with_dtype(p.dtype, "sfh_mixer_ew", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((sm_ew_kernel<T, MODE>), dim3(grid), dim3(SM_THREADS), 0, st, (const T*)a, (const T*)b, (const T*)u, (T*)y, n, vec);
  });
}

// b -> u2 (:201-204 without conv_fina's GELU).  keep_fu: the FourierUnit's blob or NULL.
int glo_fwd(const SmPlan& p, const GloParams& g, const void* bin, const Saved& s, void* keep_fu, float* rm, float* rv, void* ws, hipStream_t st) {
  void* P = p.ws.at(ws, MS_P);
  void* F = p.ws.at(ws, MS_F);
  const mi_pw_desc d1 = conv1x1(bin, p.dim, g.init_w, false, p.dim, g.init_b, nullptr, s.u1, p.C2, p.B, p.N, p.dtype);
  MI_TRY(mi_pw_gemm(&d1, p.ws.at(ws, MS_PW), st));
  MI_TRY(sm_ew_launch<EW_GELU>(p, s.u1, nullptr, nullptr, P, p.elems2, p.ew_grid2, st));
  MI_TRY(mi_fourier_unit_fwd(&p.fu, &g.fu, P, F, rm, rv, keep_fu, p.ws.at(ws, MS_FU), st));
  MI_TRY(sm_ew_launch<EW_ADD>(p, F, P, nullptr, s.r, p.elems2, p.ew_grid2, st));
  const mi_pw_desc d2 = conv1x1(s.r, p.C2, g.fina_w, false, p.C2, g.fina_b, nullptr, s.u2, p.dim, p.B, p.N, p.dtype);
  return mi_pw_gemm(&d2, p.ws.at(ws, MS_PW), st);
}

// du2 -> db (the gradient at the branch's input) and the twelve parameter gradients
int glo_bwd(const SmPlan& p, const GloParams& g, const GloGrads& gr, const void* bin, const void* du2, void* db, const Saved& s, void* ws,
            hipStream_t st) {
  const int acc = gr.fu.accumulate;
  void* dpf = p.ws.at(ws, MS_P);
  void* dr = p.ws.at(ws, MS_F);
  MI_TRY(conv1x1_bwd_input(du2, p.dim, s.r, p.C2, g.fina_w, gr.fina_w, gr.fina_b, dr, p.B, p.N, p.dtype, acc, p.ws.at(ws, MS_GRAM),
                           p.ws.at(ws, MS_CS), p.ws.at(ws, MS_PW), st, false));
  MI_TRY(mi_fourier_unit_bwd(&p.fu, &g.fu, dr, dpf, &gr.fu, s.fu, p.ws.at(ws, MS_FU), st));
  MI_TRY(sm_ew_launch<EW_ADD_DGELU>(p, dr, dpf, s.u1, dr, p.elems2, p.ew_grid2, st));
  return conv1x1_bwd_input(dr, p.C2, bin, p.dim, g.init_w, gr.init_w, gr.init_b, db, p.B, p.N, p.dtype, acc, p.ws.at(ws, MS_GRAM),
                           p.ws.at(ws, MS_CS), p.ws.at(ws, MS_PW), st, false);
}

int tail_in(const SmPlan& p, const void* l, const void* u2, void* ws, hipStream_t st) {
  void* g = p.ws.at(ws, MS_G);
  float* part = p.ws.at(ws, MS_PART);
  const int vec = sm_vec(p.N, {l, u2, g});
  return with_dtype(p.dtype, "sfh_mixer_tail_in", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((sm_tail_in<T>), dim3(p.pool, p.C2, p.B), dim3(SM_THREADS), 0, st, (const T*)l, (const T*)u2, (T*)g, part, p.dim, p.N, vec);
  });
}
int chan_attn(const SmPlan& p, const float* w1, const float* b1, const float* w2, const float* b2, const float* wc, void* ws, hipStream_t st) {
  float* sm = p.ws.at(ws, MS_SMALL);
  hipLaunchKernelGGL(sm_ca_kernel, dim3(p.B), dim3(SM_THREADS), 0, st, (const float*)p.ws.at(ws, MS_PART), w1, b1, w2, b2, wc,
                     sm + p.small_off[SMALL_M], sm + p.small_off[SMALL_HID], sm + p.small_off[SMALL_S], p.ws.at(ws, MS_FOLD), p.dim,
                     p.pool, 1.0f / (float)p.N);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

template <typename P>
GloParams glo_params(const P* q) {
  return GloParams{q->init_w, q->init_b, q->fina_w, q->fina_b,
                   mi_fourier_unit_params{q->bn_w, q->bn_b, q->fdc_w, q->fdc_b, q->gate_w, q->gate_b, q->fpe_w, q->fpe_b}};
}
template <typename G>
GloGrads glo_grads(const G* q) {
  return GloGrads{q->init_w, q->init_b, q->fina_w, q->fina_b,
                  mi_fourier_unit_grads{q->bn_w, q->bn_b, q->fdc_w, q->fdc_b, q->gate_w, q->gate_b, q->fpe_w, q->fpe_b, q->accumulate ? 1 : 0}};
}
template <typename P>
bool glo_ok(const P* q) {
  return q && q->init_w && q->init_b && q->fina_w && q->fina_b && q->bn_w && q->bn_b && q->fdc_w && q->fdc_b && q->gate_w && q->gate_b &&
         q->fpe_w && q->fpe_b;
}
template <typename P>
bool mix_ok(const P* q) {
  return q && q->cd1_w && q->cd1_b && q->cd2_w && q->cd2_b && q->cac_w && q->cac_b && q->ca1_w && q->ca1_b && q->ca2_w && q->ca2_b &&
         q->conv_w && q->conv_b;
}

}  // namespace
}  // namespace mi

using namespace mi;

// ------------------------------------------------------------------ TokenMixer_For_Gloal
extern "C" size_t mi_sfh_global_workspace(const mi_sfh_global_shape* s) {
  SmPlan p;
  return sm_check("sfh_global_workspace", SM_GLOBAL, s, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" size_t mi_sfh_global_saved_bytes(const mi_sfh_global_shape* s) {
  SmPlan p;
  return sm_check("sfh_global_saved_bytes", SM_GLOBAL, s, &p) == MI_OK ? p.saved.total : 0;
}
extern "C" int mi_sfh_global_plan(const mi_sfh_global_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "sfh_global_plan: null pointer");
  SmPlan p;
  MI_TRY(sm_check("sfh_global_plan", SM_GLOBAL, s, &p));
  return sm_plan_out(p, out);
}

extern "C" int mi_sfh_global_fwd(const mi_sfh_global_shape* s, const mi_sfh_global_params* pr, const void* x, void* out,
                                 float* running_mean, float* running_var, void* saved, void* ws, void* stream) {
  SmPlan p;
  MI_TRY(sm_check("sfh_global_fwd", SM_GLOBAL, s, &p));
  MI_CHECK_ARG(glo_ok(pr) && x && out && running_mean && running_var && ws, "sfh_global_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Saved sv = sm_saved(p, saved ? saved : p.ws.at<void>(ws, MS_SCRATCH));
  MI_TRY(glo_fwd(p, glo_params(pr), x, sv, saved ? sv.fu : nullptr, running_mean, running_var, ws, st));                  // :201-204
  return sm_ew_launch<EW_GELU>(p, sv.u2, nullptr, nullptr, out, p.elems1, p.ew_grid1, st);
}

extern "C" int mi_sfh_global_bwd(const mi_sfh_global_shape* s, const mi_sfh_global_params* pr, const void* x, const void* dout, void* dx,
                                 const mi_sfh_global_grads* gr, const void* saved, void* ws, void* stream) {
  SmPlan p;
  MI_TRY(sm_check("sfh_global_bwd", SM_GLOBAL, s, &p));
  MI_CHECK_ARG(glo_ok(pr) && x && dout && dx && gr && saved && ws, "sfh_global_bwd: null pointer");
  MI_CHECK_ARG(glo_ok(gr), "sfh_global_bwd: null gradient buffer");
  hipStream_t st = (hipStream_t)stream;
  const Saved sv = sm_saved(p, const_cast<void*>(saved));
  void* du2 = p.bw.at(p.ws.at(ws, MS_SCRATCH), BW_DU2);
  MI_TRY(sm_ew_launch<EW_DGELU>(p, dout, nullptr, sv.u2, du2, p.elems1, p.ew_grid1, st));
  return glo_bwd(p, glo_params(pr), glo_grads(gr), x, du2, dx, sv, ws, st);
}

// ------------------------------------------------------------------ Mixer
extern "C" size_t mi_sfh_mixer_workspace(const mi_sfh_mixer_shape* s) {
  SmPlan p;
  return sm_check("sfh_mixer_workspace", SM_MIXER, s, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" size_t mi_sfh_mixer_saved_bytes(const mi_sfh_mixer_shape* s) {
  SmPlan p;
  return sm_check("sfh_mixer_saved_bytes", SM_MIXER, s, &p) == MI_OK ? p.saved.total : 0;
}
extern "C" int mi_sfh_mixer_plan(const mi_sfh_mixer_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "sfh_mixer_plan: null pointer");
  SmPlan p;
  MI_TRY(sm_check("sfh_mixer_plan", SM_MIXER, s, &p));
  return sm_plan_out(p, out);
}

extern "C" int mi_sfh_mixer_fwd(const mi_sfh_mixer_shape* s, const mi_sfh_mixer_params* pr, const void* x, void* out, float* running_mean,
                                float* running_var, void* saved, void* ws, void* stream) {
  SmPlan p;
  MI_TRY(sm_check("sfh_mixer_fwd", SM_MIXER, s, &p));
  MI_CHECK_ARG(glo_ok(pr) && mix_ok(pr) && x && out && running_mean && running_var && ws, "sfh_mixer_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int dim = p.dim, C2 = p.C2;
  const Saved sv = sm_saved(p, saved ? saved : p.ws.at<void>(ws, MS_SCRATCH));
  const mi_pw_desc di = init_desc(x, pr->conv_w, pr->conv_b, sv.a,
                                  (int64_t)((p.saved.off[SV_B] - p.saved.off[SV_A]) / dtype_size(p.dtype)), dim, p.B, p.N, p.dtype);
  MI_TRY(mi_pw_gemm(&di, p.ws.at(ws, MS_PW), st));                                                                            // :240-241
  const mi_sfh_local_params lp = {pr->cd1_w, pr->cd1_b, pr->cd2_w, pr->cd2_b};
  MI_TRY(mi_sfh_local_fwd(&p.loc, &lp, sv.a, sv.l, p.ws.at(ws, MS_LOCAL), st));                                              // :242
  MI_TRY(glo_fwd(p, glo_params(pr), sv.b, sv, saved ? sv.fu : nullptr, running_mean, running_var, ws, st));                 // :243
  MI_TRY(tail_in(p, sv.l, sv.u2, ws, st));                                                                                   // :244-245
  MI_TRY(chan_attn(p, pr->ca1_w, pr->ca1_b, pr->ca2_w, pr->ca2_b, pr->cac_w, ws, st));                                       // :246
  const mi_pw_desc dc = per_image(conv1x1(p.ws.at(ws, MS_G), C2, (const float*)p.ws.at(ws, MS_FOLD), false, C2, pr->cac_b, nullptr, out, dim,
                                          p.B, p.N, p.dtype));
  return mi_pw_gemm(&dc, p.ws.at(ws, MS_PW), st);                                                                             // :247
}

extern "C" int mi_sfh_mixer_bwd(const mi_sfh_mixer_shape* s, const mi_sfh_mixer_params* pr, const void* x, const void* dout, void* dx,
                                const mi_sfh_mixer_grads* gr, const void* saved, void* ws, void* stream) {
  SmPlan p;
  MI_TRY(sm_check("sfh_mixer_bwd", SM_MIXER, s, &p));
  MI_CHECK_ARG(glo_ok(pr) && mix_ok(pr) && x && dout && dx && gr && saved && ws, "sfh_mixer_bwd: null pointer");
  MI_CHECK_ARG(glo_ok(gr) && mix_ok(gr), "sfh_mixer_bwd: null gradient buffer");
  hipStream_t st = (hipStream_t)stream;
  const int dim = p.dim, C2 = p.C2, acc = gr->accumulate ? 1 : 0, dt = p.dtype;
  const Saved sv = sm_saved(p, const_cast<void*>(saved));
  void* bw = p.ws.at(ws, MS_SCRATCH);
  void* e = p.bw.at(bw, BW_E);
  void* dl = p.bw.at(bw, BW_DL);
  void* du2 = p.bw.at(bw, BW_DU2);
  void* dA = p.bw.at(bw, BW_DA);
  void* dB = p.bw.at(bw, BW_DB);
  void* g = p.ws.at(ws, MS_G);
  float* sm = p.ws.at(ws, MS_SMALL);
  float* fold = p.ws.at(ws, MS_FOLD);
  float* P = p.ws.at(ws, MS_PGRAM);
  // g, m, hidden, s and the folded weights again, by the forward's own kernels (bit for bit the forward's)
  MI_TRY(tail_in(p, sv.l, sv.u2, ws, st));
  MI_TRY(chan_attn(p, pr->ca1_w, pr->ca1_b, pr->ca2_w, pr->ca2_b, pr->cac_w, ws, st));
  MI_TRY(launch_chan_sum(dout, gr->cac_b, p.B, dim, p.N, dt, acc, p.ws.at(ws, MS_CS), st));
  const mi_gram_desc pg = wgrad_gram(dout, dim, g, C2, p.B, p.N, dt, P, 0, 0);
  MI_TRY(mi_gram(&pg, p.ws.at(ws, MS_GRAM), st));
  hipLaunchKernelGGL(sm_gate_bwd, dim3(p.B), dim3(SM_THREADS), 0, st, (const float*)P, pr->cac_w, pr->ca1_w, pr->ca2_w,
                     (const float*)(sm + p.small_off[SMALL_HID]), (const float*)(sm + p.small_off[SMALL_S]), sm + p.small_off[SMALL_DZ2],
                     sm + p.small_off[SMALL_DZ1], sm + p.small_off[SMALL_DMN], dim, 1.0f / (float)p.N);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(sm_gate_wgrad, dim3(cdiv(3 * dim * C2 + C2 + dim, SM_THREADS)), dim3(SM_THREADS), 0, st, (const float*)P,
                     (const float*)(sm + p.small_off[SMALL_M]), (const float*)(sm + p.small_off[SMALL_HID]),
                     (const float*)(sm + p.small_off[SMALL_S]), (const float*)(sm + p.small_off[SMALL_DZ2]),
                     (const float*)(sm + p.small_off[SMALL_DZ1]), gr->cac_w, gr->ca1_w, gr->ca1_b, gr->ca2_w, gr->ca2_b, p.B, dim, acc);
  MI_LAUNCH_CHECK();
  const mi_pw_desc de = per_image(conv1x1(dout, dim, fold, true, C2, nullptr, nullptr, e, C2, p.B, p.N, dt));
  MI_TRY(mi_pw_gemm(&de, p.ws.at(ws, MS_PW), st));
  const int vec = sm_vec(p.N, {e, sv.l, sv.u2, dl, du2});
  MI_TRY(with_dtype(dt, "sfh_mixer_tail_back", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((sm_tail_back<T>), dim3(p.tail_grid, C2, p.B), dim3(SM_THREADS), 0, st, (const T*)e, (const T*)sv.l, (const T*)sv.u2,
                       (const float*)(sm + p.small_off[SMALL_DMN]), (T*)dl, (T*)du2, dim, p.N, vec);
  }));
  const mi_sfh_local_params lp = {pr->cd1_w, pr->cd1_b, pr->cd2_w, pr->cd2_b};
  const mi_sfh_local_grads lg = {gr->cd1_w, gr->cd1_b, gr->cd2_w, gr->cd2_b, acc};
  MI_TRY(mi_sfh_local_bwd(&p.loc, &lp, sv.a, dl, dA, &lg, p.ws.at(ws, MS_LOCAL), st));
  MI_TRY(glo_bwd(p, glo_params(pr), glo_grads(gr), sv.b, du2, dB, sv, ws, st));
  // conv_init: the two halves of its gradient stay apart (two Grams, two bias sums); dx takes them as the two K panels
  const mi_gram_desc ga = wgrad_gram(dA, dim, x, dim, p.B, p.N, dt, gr->conv_w, acc);
  MI_TRY(mi_gram(&ga, p.ws.at(ws, MS_GRAM), st));
  const mi_gram_desc gb = wgrad_gram(dB, dim, x, dim, p.B, p.N, dt, gr->conv_w + (size_t)dim * dim, acc);
  MI_TRY(mi_gram(&gb, p.ws.at(ws, MS_GRAM), st));
  MI_TRY(launch_chan_sum(dA, gr->conv_b, p.B, dim, p.N, dt, acc, p.ws.at(ws, MS_CS), st));
  MI_TRY(launch_chan_sum(dB, gr->conv_b + dim, p.B, dim, p.N, dt, acc, p.ws.at(ws, MS_CS), st));
  mi_pw_desc dxd = conv1x1(dA, dim, pr->conv_w, true, dim, nullptr, nullptr, dx, dim, p.B, p.N, dt);
  dxd.x2 = dB; dxd.x2_bs = dxd.x1_bs; dxd.k2 = dim;
  return mi_pw_gemm(&dxd, p.ws.at(ws, MS_PW), st);
}
