// SFHformer's FourierUnit (SFHformer.py:143-180): what sits between the two real 2-D transforms of dft2.hip.   fp32 between the
// input load and the output store.
//
//   c channels, C2 = 2c, K = W/2 + 1, N = H K bins per plane, G groups, S = C2 / G, alpha = 1/sqrt(HW)
//   Z  = rfft2(x) unnormalised (dft2_r2c_run), planar Re | Im [B,c,N]; the reference's interleaved channel j = 2i + d (d = 0: Re Z_i,
//        d = 1: Im Z_i) is pure indexing here: the middle works on channels in PLANAR order p = d c + i, j(p) = 2 (p mod c) + p / c,
//        and every parameter is read at j(p).  No interleaved copy is made.
//   BN   the reference normalises alpha Z.  With mu, var the batch statistics of the RAW Z (per channel over n = B N bins):
//        xhat = (alpha z - alpha mu) / sqrt(alpha^2 var + eps) = (z - mu) r,  r = alpha / sqrt(alpha^2 var + eps):  the ortho scale is
//        folded into r exactly (eps is not rescaled).  running_mean <- (1 - mom) rm + mom alpha mu,  running_var <- (1 - mom) rv +
//        mom alpha^2 var n / (n - 1).  Eval: mu = rm / alpha, r = alpha / sqrt(rv + eps).
//        Variance: every workgroup takes one chunk of one plane, sums it, forms ITS mean, and sums the squares of the deviations
//        from that mean (second read of the chunk); one thread per channel then merges the (count, mean, M2) triples in a fixed
//        order with Chan's update.  No sum of squares is ever subtracted from a squared sum: the DC-heavy Re channels lose nothing.
//   t  = fpe(t1) + t1,  t1 = gamma xhat + beta: depthwise 3x3, zero padding, bias, over the (H, K) plane: one kernel that reads Z
//        (t1 is never stored; the padding is of t1, so a neighbour outside the plane adds 0, not beta).
//   s  = softmax_g(Ww t + bw);  ts[j] = s_{g(j)} t[j], g(j) = j / S                                   (one kernel, one thread per bin)
//   pre = W' ts + sum_g s_g bfdc[g C2 + k],  W'[k, g S + jl] = fdc.weight[g C2 + k, jl]: ONE dense C2 x C2 product (mi_pw_gemm at
//        fp32: the fp32 MFMA) on the gate-scaled input; the [B, G C2, H, K] tensor of the grouped conv does not exist.
//   o  = sqrt(HW) gelu_erf(pre), stored planar Re | Im [B,c,N];  out = dft2_c2r_run(o) = irfft2(gelu(pre), norm='ortho')
// Backward: do = (adjoint of c2r)(dout) sqrt(HW);  dpre = gelu'(pre) do;  dW' = sum dpre (x) ts (mi_gram) and q = W'^T dpre
// (mi_pw_gemm);  dbfdc[g C2 + k] = sum s_g dpre[k] (mi_gram);  ds_g = sum_{j in g} t_j q_j + sum_k bfdc[g C2 + k] dpre[k];
// dlogit = s (ds - s . ds);  dt = s_{g(j)} q_j + Ww^T dlogit;  dWw = sum dlogit (x) t (mi_gram), dbw = sum dlogit (channel sum);
// dt1 = dt + fpe^T dt;  dfpe.weight[tap] = sum dt t1(shifted), dfpe.bias = sum dt, dgamma = sum dt1 xhat, dbeta = sum dt1 (per-
// workgroup partial rows summed in a fixed order);  dz = r gamma (dt1 - mean(dt1) - xhat mean(dt1 xhat)) in training mode,
// r gamma dt1 in eval mode;  dx = (adjoint of r2c)(dz).  No atomics anywhere: bitwise reproducible.
// Saved for the backward: Z and the per-channel (mu, r).  t, s, ts and pre are recomputed from them by the forward's own kernels.
// sfh_plan is the ONE place that decides sections, grids and launch counts.
#include <limits.h>

#include "dft2.h"

namespace mi {
namespace {

constexpr int SFH_THREADS = 256, SFH_CHUNK = 2048, SFH_MAX_C = 256, SFH_MAX_G = 8, SFH_MIN_HW = 2, SFH_MAX_HW = 512;
constexpr int SFH_EW = 1024;   // elements of one plane a workgroup of the per-element passes takes (4 per thread)
constexpr int SFH_GB = 64;     // bins (threads) of a workgroup of the gate kernels: one wave, so that few bins still spread over the chip
constexpr int SFH_RED = 12;    // rows of the fpe / BatchNorm backward partials: 9 taps, fpe bias, dgamma, dbeta

// Where channel ch of a planar tensor lives and which parameter it reads: ch = half * Ch + i sits at half * hs + i * cs (+ b * bs)
// and reads parameter i * ps + half.  The spectrum: Ch = c, hs = B c N, cs = N, bs = c N, ps = 2.  A plain [B,C,N]: Ch = C, ps = 1.
struct ChanMap {
  int C, Ch, ps; int64_t hs, cs, bs;
  __host__ __device__ int64_t off(int ch) const { return (int64_t)(ch / Ch) * hs + (int64_t)(ch % Ch) * cs; }
  __host__ __device__ int par(int ch) const { return (ch % Ch) * ps + ch / Ch; }
};

enum { SS_DFT = 0, SS_T, SS_Z, SS_U, SS_A, SS_B, SS_P, SS_Q, SS_S, SS_DL, SS_STAT, SS_BNP, SS_WP, SS_GT, SS_RP, SS_PW, SS_GRAM, SS_CS,
       SFH_SECTIONS };

struct SfhPlan {
  int B, c, C2, G, S, H, W, K, N;
  Dft2Geom dft; Dft2Blob dft_blob;    // the transforms' tiles and grids; their blob (SS_DFT: its tables, SS_T: its intermediate)
  int nchunk, nparts;                 // chunks of a plane; partials per channel (B * nchunk)
  int64_t elems, bins;                // B C2 N; B N
  int nblk, grid_elems, grid_bins, grid_chan, grid_w, grid_scatter, grid_fin;
  int kernels_fwd, kernels_bwd, lib_calls_fwd, lib_calls_bwd;
  Sections<SFH_SECTIONS> ws;
  Sections<2> saved;                  // the blob: Z, then (mu, r)
  ChanMap map;
};

bool sfh_plan(int B, int c, int G, int H, int W, SfhPlan* p) {
  *p = SfhPlan{};
  if (B <= 0 || c < 1 || c > SFH_MAX_C || G < 1 || G > SFH_MAX_G || (2 * c) % G) return false;
  if (H < SFH_MIN_HW || W < SFH_MIN_HW || H > SFH_MAX_HW || W > SFH_MAX_HW) return false;
  const int K = W / 2 + 1, C2 = 2 * c, N = H * K;
  const int64_t elems = (int64_t)B * C2 * N;
  if (elems > INT_MAX || (int64_t)B * C2 * cdiv(N, SFH_EW) > INT_MAX) return false;
  if (!dft2_geom((int64_t)B * c, H, W, &p->dft) || !dft2_blob(p->dft, &p->dft_blob)) return false;
  p->B = B; p->c = c; p->C2 = C2; p->G = G; p->S = C2 / G; p->H = H; p->W = W; p->K = K; p->N = N;
  p->nchunk = cdiv(N, SFH_CHUNK); p->nparts = B * p->nchunk;
  p->elems = elems; p->bins = (int64_t)B * N;
  p->nblk = cdiv(N, SFH_EW);
  p->grid_elems = B * C2 * p->nblk; p->grid_bins = cdiv(p->bins, SFH_GB); p->grid_chan = cdiv(C2, SFH_THREADS);
  p->grid_w = cdiv((int64_t)C2 * C2, SFH_THREADS); p->grid_scatter = cdiv((int64_t)C2 * C2 + 2 * G * C2, SFH_THREADS);
  p->grid_fin = cdiv((int64_t)C2 * SFH_RED, SFH_THREADS);
  p->map = ChanMap{C2, c, 2, (int64_t)B * c * N, (int64_t)N, (int64_t)c * N};
  // forward: tables, r2c (2), BN partials, BN finish, W', t, gate, gelu, c2r (2); one 1x1 product
  // backward: tables, the c2r adjoint (2), W', t, gate, gelu', gate backward, fpe / BN partials, their finish, dz, the gradient
  // scatter, the r2c adjoint (2); the 1x1 product again, W'^T dpre, three Grams and a channel sum
  p->kernels_fwd = 11; p->kernels_bwd = 14; p->lib_calls_fwd = 1; p->lib_calls_bwd = 6;
  const size_t spec = (size_t)elems * 4, gate = (size_t)p->bins * G * 4;
  Sections<SFH_SECTIONS>& ws = p->ws;
  ws.put(SS_DFT, p->dft_blob.t); ws.put(SS_T, spec);   // together the transforms' blob: its tables, then its complex intermediate
  ws.put(SS_Z, spec); ws.put(SS_U, spec); ws.put(SS_A, spec); ws.put(SS_B, spec); ws.put(SS_P, spec); ws.put(SS_Q, spec);
  ws.put(SS_S, gate); ws.put(SS_DL, gate);
  ws.put(SS_STAT, (size_t)4 * C2 * 4);
  ws.put(SS_BNP, (size_t)C2 * p->nparts * 2 * 4);
  ws.put(SS_WP, (size_t)C2 * C2 * 4);
  ws.put(SS_GT, ((size_t)C2 * C2 + (size_t)2 * G * C2) * 4);
  ws.put(SS_RP, (size_t)C2 * p->nparts * SFH_RED * 4);
  ws.put(SS_PW, max_of({pw_ws_bytes(probe1x1(C2, C2, false, B, N, MI_F32)), pw_ws_bytes(probe1x1(C2, C2, true, B, N, MI_F32))}));
  ws.put(SS_GRAM, max_of({gram_ws_bytes(probe_wgrad(C2, C2, B, N, MI_F32)), gram_ws_bytes(probe_wgrad(G, C2, B, N, MI_F32))}));
  ws.put(SS_CS, chan_sum_workspace(G, N));
  p->saved.put(0, spec); p->saved.put(1, (size_t)2 * C2 * 4);
  return true;
}

// Sum over the 256 threads in a fixed order (wave sums on the VALU, then the four of them); every thread gets the total.
__device__ __forceinline__ float block_sum(float v, float* lds) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// n = h K + l without an integer division: n < 2^24 is exact in fp32 and the rounded quotient is off by at most one.
__device__ __forceinline__ void split_hl(int n, int K, float inv_k, int& h, int& l) {
  h = (int)((float)n * inv_k);
  l = n - h * K;
  if (l < 0) { --h; l += K; } else if (l >= K) { ++h; l -= K; }
}

// The per-element passes: workgroup blockIdx.x takes SFH_EW consecutive bins of ONE plane (image b, planar channel p), so the
// channel's constants and addresses are wave-uniform and no thread divides.
struct PlaneBlock { int b, p, n0; };
__device__ __forceinline__ PlaneBlock plane_block(int C, int nblk) {
  const int plane = blockIdx.x / nblk;
  return PlaneBlock{plane / C, plane % C, (int)(blockIdx.x - plane * nblk) * SFH_EW};
}

// ---------------------------------------------------------------------------------------------------------------- BatchNorm
// grid (nparts, C): workgroup (part, ch) takes chunk part % nchunk of plane (part / nchunk, ch): its mean and the sum of squared
// deviations from that mean.
__global__ __launch_bounds__(SFH_THREADS) void bn_partial_kernel(const float* __restrict__ x, ChanMap m, int N, int nchunk,
                                                                 float* __restrict__ part) {
  __shared__ float lds[4];
  const int ch = blockIdx.y, b = blockIdx.x / nchunk, k = blockIdx.x - b * nchunk;
  const int n0 = k * SFH_CHUNK, n1 = min(N, n0 + SFH_CHUNK);
  const float* src = x + m.off(ch) + (int64_t)b * m.bs;
  float s = 0.f;
  for (int n = n0 + threadIdx.x; n < n1; n += SFH_THREADS) s += src[n];
  const float mean = block_sum(s, lds) / (float)(n1 - n0);
  float q = 0.f;
  for (int n = n0 + threadIdx.x; n < n1; n += SFH_THREADS) { const float d = src[n] - mean; q += d * d; }
  q = block_sum(q, lds);
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)ch * gridDim.x + blockIdx.x) * 2;
    o[0] = mean; o[1] = q;
  }
}

// One thread per channel.  Training: merges the partials in order (Chan), writes (mu, r) and updates the running statistics in
// place.  Eval: (mu, r) from the running statistics.  alpha: the scale the caller's normalisation sees its input through.
__global__ __launch_bounds__(SFH_THREADS) void bn_finish_kernel(const float* __restrict__ part, ChanMap m, int N, int nchunk,
                                                                int nparts, float alpha, float eps, float momentum, int training,
                                                                float* __restrict__ rmean, float* __restrict__ rvar,
                                                                float* __restrict__ stat) {
  const int ch = blockIdx.x * SFH_THREADS + threadIdx.x;
  if (ch >= m.C) return;
  const int j = m.par(ch);
  float mu, r;
  if (training) {
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int i = 0; i < nparts; ++i) {
      const int k = i % nchunk;
      const float nb = (float)(min(N, (k + 1) * SFH_CHUNK) - k * SFH_CHUNK);
      const float mb = part[((int64_t)ch * nparts + i) * 2], qb = part[((int64_t)ch * nparts + i) * 2 + 1];
      const float tot = cnt + nb, d = mb - mean;
      mean += d * (nb / tot);
      m2 += qb + d * d * (cnt * nb / tot);
      cnt = tot;
    }
    const float var = m2 / cnt;
    mu = mean; r = alpha / sqrtf(alpha * alpha * var + eps);
    rmean[j] = (1.f - momentum) * rmean[j] + momentum * (alpha * mean);
    rvar[j] = (1.f - momentum) * rvar[j] + momentum * (alpha * alpha * var * (cnt / fmaxf(cnt - 1.f, 1.f)));
  } else {
    mu = rmean[j] / alpha; r = alpha / sqrtf(rvar[j] + eps);
  }
  stat[ch] = mu; stat[m.C + ch] = r;
}

// t = fpe(t1) + t1 with t1 = gamma (z - mu) r + beta formed on the fly; t [B][C][H][K]
__global__ __launch_bounds__(SFH_THREADS) void bn_fpe_kernel(const float* __restrict__ z, ChanMap m, const float* __restrict__ stat,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ fw, const float* __restrict__ fb,
                                                             float* __restrict__ t, int H, int K, int nblk) {
  const int N = H * K;
  const PlaneBlock pb = plane_block(m.C, nblk);
  const int j = m.par(pb.p);
  const float* src = z + m.off(pb.p) + (int64_t)pb.b * m.bs;
  float* dst = t + ((int64_t)pb.b * m.C + pb.p) * N;
  const float mu = stat[pb.p], r = stat[m.C + pb.p], g = gamma[j], be = beta[j], bias = fb[j], inv_k = 1.f / (float)K;
  float w[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) w[i] = fw[j * 9 + i];
#pragma unroll
  for (int i = 0; i < SFH_EW / SFH_THREADS; ++i) {
    const int n = pb.n0 + i * SFH_THREADS + threadIdx.x;
    if (n >= N) break;
    int h, l;
    split_hl(n, K, inv_k, h, l);
    float acc = bias, centre = 0.f;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
      for (int e = -1; e <= 1; ++e) {
        const int hh = h + a, ll = l + e;
        if (hh >= 0 && hh < H && ll >= 0 && ll < K) {
          const float v = g * ((src[hh * K + ll] - mu) * r) + be;
          acc += w[(a + 1) * 3 + (e + 1)] * v;
          if (a == 0 && e == 0) centre = v;
        }
      }
    dst[n] = acc + centre;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the mix
// W'[p][p'] (planar order on both sides) from fdc.weight [G C2][S]
__global__ __launch_bounds__(SFH_THREADS) void sfh_fold_kernel(const float* __restrict__ fdcw, ChanMap m, int S, float* __restrict__ wp) {
  const int e = blockIdx.x * SFH_THREADS + threadIdx.x;
  if (e >= m.C * m.C) return;
  const int k = m.par(e / m.C), j = m.par(e % m.C), g = j / S;
  wp[e] = fdcw[((int64_t)g * m.C + k) * S + (j - g * S)];
}

// One thread per bin, one wave per workgroup: the G gate logits (channels summed in planar order), their softmax, ts = s_{g(j)} t.
template <int G>
__global__ __launch_bounds__(SFH_GB) void sfh_gate_kernel(const float* __restrict__ t, ChanMap m, int S, const float* __restrict__ ww,
                                                          const float* __restrict__ bw, float* __restrict__ s, float* __restrict__ ts,
                                                          int N, int bins) {
  const int idx = blockIdx.x * SFH_GB + threadIdx.x;
  if (idx >= bins) return;
  const int b = idx / N, n = idx - b * N, C = m.C;
  const float* tb = t + (int64_t)b * C * N + n;
  float acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = bw[g];
#pragma unroll 4
  for (int p = 0; p < C; ++p) {
    const float v = tb[(int64_t)p * N];
    const int j = m.par(p);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] += ww[g * C + j] * v;
  }
  float mx = acc[0];
#pragma unroll
  for (int g = 1; g < G; ++g) mx = fmaxf(mx, acc[g]);
  float den = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) { acc[g] = expf(acc[g] - mx); den += acc[g]; }
#pragma unroll
  for (int g = 0; g < G; ++g) { acc[g] = acc[g] / den; s[((int64_t)b * G + g) * N + n] = acc[g]; }
  float* ob = ts + (int64_t)b * C * N + n;
#pragma unroll 4
  for (int p = 0; p < C; ++p) {
    const int gsel = m.par(p) / S;
    float sv = acc[0];
#pragma unroll
    for (int g = 1; g < G; ++g) sv = gsel == g ? acc[g] : sv;
    ob[(int64_t)p * N] = sv * tb[(int64_t)p * N];
  }
}

// o = scale gelu_erf(pre + the bias product on s), stored planar Re | Im
__global__ __launch_bounds__(SFH_THREADS) void sfh_gelu_kernel(const float* __restrict__ pre, const float* __restrict__ s,
                                                               const float* __restrict__ bfdc, ChanMap m, int G, float* __restrict__ o,
                                                               float scale, int N, int nblk) {
  const PlaneBlock pb = plane_block(m.C, nblk);
  const int j = m.par(pb.p);
  const float* src = pre + ((int64_t)pb.b * m.C + pb.p) * N;
  const float* sb = s + (int64_t)pb.b * G * N;
  float* dst = o + m.off(pb.p) + (int64_t)pb.b * m.bs;
#pragma unroll
  for (int i = 0; i < SFH_EW / SFH_THREADS; ++i) {
    const int n = pb.n0 + i * SFH_THREADS + threadIdx.x;
    if (n >= N) break;
    float v = src[n];
    for (int g = 0; g < G; ++g) v += sb[(int64_t)g * N + n] * bfdc[g * m.C + j];
    dst[n] = scale * (0.5f * v * (1.f + erff(v * 0.70710678118654752440f)));
  }
}

// dpre = gelu'(pre + the bias product) * scale * g (g planar Re | Im), over pre in place
__global__ __launch_bounds__(SFH_THREADS) void sfh_gelu_bwd_kernel(float* __restrict__ pre, const float* __restrict__ s,
                                                                   const float* __restrict__ bfdc, ChanMap m, int G,
                                                                   const float* __restrict__ g, float scale, int N, int nblk) {
  const PlaneBlock pb = plane_block(m.C, nblk);
  const int j = m.par(pb.p);
  float* io = pre + ((int64_t)pb.b * m.C + pb.p) * N;
  const float* sb = s + (int64_t)pb.b * G * N;
  const float* gsrc = g + m.off(pb.p) + (int64_t)pb.b * m.bs;
#pragma unroll
  for (int i = 0; i < SFH_EW / SFH_THREADS; ++i) {
    const int n = pb.n0 + i * SFH_THREADS + threadIdx.x;
    if (n >= N) break;
    float v = io[n];
    for (int q = 0; q < G; ++q) v += sb[(int64_t)q * N + n] * bfdc[q * m.C + j];
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f)), pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
    io[n] = (cdf + v * pdf) * (scale * gsrc[n]);
  }
}

// One thread per bin, one wave per workgroup: ds, the softmax backward, dt = s_{g(j)} q + Ww^T dlogit over q in place.
template <int G>
__global__ __launch_bounds__(SFH_GB) void sfh_gate_bwd_kernel(const float* __restrict__ t, float* __restrict__ q,
                                                              const float* __restrict__ dpre, const float* __restrict__ s, ChanMap m,
                                                              int S, const float* __restrict__ ww, const float* __restrict__ bfdc,
                                                              float* __restrict__ dl, int N, int bins) {
  const int idx = blockIdx.x * SFH_GB + threadIdx.x;
  if (idx >= bins) return;
  const int b = idx / N, n = idx - b * N, C = m.C;
  const int64_t base = (int64_t)b * C * N + n;
  float ds[G], sv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) { ds[g] = 0.f; sv[g] = s[((int64_t)b * G + g) * N + n]; }
#pragma unroll 4
  for (int p = 0; p < C; ++p) {
    const int j = m.par(p), gsel = j / S;
    const float tq = t[base + (int64_t)p * N] * q[base + (int64_t)p * N], dp = dpre[base + (int64_t)p * N];
#pragma unroll
    for (int g = 0; g < G; ++g) ds[g] += (gsel == g ? tq : 0.f) + bfdc[g * C + j] * dp;
  }
  float dot = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) dot += sv[g] * ds[g];
#pragma unroll
  for (int g = 0; g < G; ++g) { ds[g] = sv[g] * (ds[g] - dot); dl[((int64_t)b * G + g) * N + n] = ds[g]; }
#pragma unroll 4
  for (int p = 0; p < C; ++p) {
    const int j = m.par(p), gsel = j / S;
    float sg = sv[0];
#pragma unroll
    for (int g = 1; g < G; ++g) sg = gsel == g ? sv[g] : sg;
    float acc = sg * q[base + (int64_t)p * N];
#pragma unroll
    for (int g = 0; g < G; ++g) acc += ww[g * C + j] * ds[g];
    q[base + (int64_t)p * N] = acc;
  }
}

// ---------------------------------------------------------------------------------------- backward of fpe + residual and of BN
// grid (nparts, C), the chunks of bn_partial_kernel.  dt1 = dt + fpe^T dt is stored; the twelve per-channel sums of the chunk go to
// part[ch][part][12]: dfpe.weight's nine taps (dt times the shifted t1, recomputed from z), sum dt, sum dt1 xhat, sum dt1.
__global__ __launch_bounds__(SFH_THREADS) void fpe_bn_bwd_partial_kernel(const float* __restrict__ dt, const float* __restrict__ z,
                                                                         ChanMap m, const float* __restrict__ stat,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         const float* __restrict__ fw, float* __restrict__ dt1,
                                                                         float* __restrict__ part, int H, int K, int nchunk) {
  __shared__ float lds[4][SFH_RED];
  const int N = H * K;
  const int ch = blockIdx.y, b = blockIdx.x / nchunk, k = blockIdx.x - b * nchunk;
  const int n0 = k * SFH_CHUNK, n1 = min(N, n0 + SFH_CHUNK);
  const int j = m.par(ch);
  const float inv_k = 1.f / (float)K;
  const float* src = z + m.off(ch) + (int64_t)b * m.bs;
  const float* dsrc = dt + ((int64_t)b * m.C + ch) * N;
  float* ddst = dt1 + ((int64_t)b * m.C + ch) * N;
  const float mu = stat[ch], r = stat[m.C + ch], g = gamma[j], be = beta[j];
  float w[9], acc[SFH_RED];
#pragma unroll
  for (int i = 0; i < 9; ++i) w[i] = fw[j * 9 + i];
#pragma unroll
  for (int i = 0; i < SFH_RED; ++i) acc[i] = 0.f;
  for (int n = n0 + threadIdx.x; n < n1; n += SFH_THREADS) {
    int h, l;
    split_hl(n, K, inv_k, h, l);
    const float d = dsrc[n];
    float d1 = d;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
      for (int e = -1; e <= 1; ++e) {
        const int i = (a + 1) * 3 + (e + 1);
        const int hf = h + a, lf = l + e;           // the input the forward tap read
        if (hf >= 0 && hf < H && lf >= 0 && lf < K) acc[i] += d * (g * ((src[hf * K + lf] - mu) * r) + be);
        const int hb = h - a, lb = l - e;           // the output this input fed through that tap
        if (hb >= 0 && hb < H && lb >= 0 && lb < K) d1 += w[i] * dsrc[hb * K + lb];
      }
    ddst[n] = d1;
    acc[9] += d;
    acc[10] += d1 * ((src[n] - mu) * r);
    acc[11] += d1;
  }
  // the twelve sums: wave sums on the VALU, then the four waves' in a fixed order, one barrier for all twelve
#pragma unroll
  for (int i = 0; i < SFH_RED; ++i) {
    const float v = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < SFH_RED)
    part[((int64_t)ch * gridDim.x + blockIdx.x) * SFH_RED + threadIdx.x] =
        (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
}

// One thread per (channel, row): the partials summed in order, into the parameter gradients; the two means of the BN backward.
__global__ __launch_bounds__(SFH_THREADS) void fpe_bn_bwd_finish_kernel(const float* __restrict__ part, ChanMap m, int nparts,
                                                                        float inv_n, int accumulate, float* __restrict__ g_fw,
                                                                        float* __restrict__ g_fb, float* __restrict__ g_gamma,
                                                                        float* __restrict__ g_beta, float* __restrict__ means) {
  const int e = blockIdx.x * SFH_THREADS + threadIdx.x;
  if (e >= m.C * SFH_RED) return;
  const int ch = e / SFH_RED, i = e - ch * SFH_RED, j = m.par(ch);
  float v = 0.f;
  for (int k = 0; k < nparts; ++k) v += part[((int64_t)ch * nparts + k) * SFH_RED + i];
  float* dst = i < 9 ? g_fw + j * 9 + i : i == 9 ? g_fb + j : i == 10 ? g_gamma + j : g_beta + j;
  *dst = accumulate ? *dst + v : v;
  if (i == 11) means[ch] = v * inv_n;
  if (i == 10) means[m.C + ch] = v * inv_n;
}

// dz = r gamma (dt1 - mean(dt1) - xhat mean(dt1 xhat)) (training) / r gamma dt1 (eval), stored planar Re | Im
__global__ __launch_bounds__(SFH_THREADS) void bn_bwd_dz_kernel(const float* __restrict__ dt1, const float* __restrict__ z, ChanMap m,
                                                                const float* __restrict__ stat, const float* __restrict__ means,
                                                                const float* __restrict__ gamma, int training,
                                                                float* __restrict__ dz, int N, int nblk) {
  const PlaneBlock pb = plane_block(m.C, nblk);
  const int64_t o = m.off(pb.p) + (int64_t)pb.b * m.bs;
  const float* src = dt1 + ((int64_t)pb.b * m.C + pb.p) * N;
  const float mu = stat[pb.p], r = stat[m.C + pb.p], rg = r * gamma[m.par(pb.p)];
  const float m1 = training ? means[pb.p] : 0.f, m2 = training ? means[m.C + pb.p] : 0.f;
#pragma unroll
  for (int i = 0; i < SFH_EW / SFH_THREADS; ++i) {
    const int n = pb.n0 + i * SFH_THREADS + threadIdx.x;
    if (n >= N) break;
    float d = src[n];
    if (training) d = d - m1 - ((z[o + n] - mu) * r) * m2;
    dz[o + n] = rg * d;
  }
}

// dW' [C][C], dbfdc [G][C], dWw [G][C] (planar order) -> the gradients in the reference's layouts, added or written
__global__ __launch_bounds__(SFH_THREADS) void sfh_scatter_kernel(const float* __restrict__ tmp, ChanMap m, int G, int S, int accumulate,
                                                                  float* __restrict__ g_fdcw, float* __restrict__ g_fdcb,
                                                                  float* __restrict__ g_ww) {
  const int e = blockIdx.x * SFH_THREADS + threadIdx.x;
  const int C = m.C, cc = C * C;
  if (e >= cc + 2 * G * C) return;
  float* dst;
  if (e < cc) {
    const int k = m.par(e / C), j = m.par(e % C), g = j / S;
    dst = g_fdcw + ((int64_t)g * C + k) * S + (j - g * S);
  } else {
    const int r = (e - cc) % (G * C), g = r / C, j = m.par(r % C);
    dst = (e - cc < G * C ? g_fdcb : g_ww) + g * C + j;
  }
  *dst = accumulate ? *dst + tmp[e] : tmp[e];
}

template <int G, typename... A> void launch_gate(dim3 grid, hipStream_t st, A... a) {
  hipLaunchKernelGGL(sfh_gate_kernel<G>, grid, dim3(SFH_GB), 0, st, a...);
}
template <int G, typename... A> void launch_gate_bwd(dim3 grid, hipStream_t st, A... a) {
  hipLaunchKernelGGL(sfh_gate_bwd_kernel<G>, grid, dim3(SFH_GB), 0, st, a...);
}
#define SFH_FOR_G(G, CALL)                                                                                         \
  switch (G) {                                                                                                     \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;               \
  }

int sfh_check(const char* who, const mi_fourier_unit_shape* s, SfhPlan* p) {
  MI_CHECK_ARG(s, "%s: null shape", who);
  MI_CHECK_ARG(s->dtype == MI_F32 || s->dtype == MI_BF16, "%s: bad dtype %d", who, s->dtype);
  MI_CHECK_ARG(s->B > 0, "%s: bad shape B=%d", who, s->B);
  MI_CHECK_ARG(s->c >= 1 && s->c <= SFH_MAX_C, "%s: c=%d outside the supported 1..%d", who, s->c, SFH_MAX_C);
  MI_CHECK_ARG(s->groups >= 1 && s->groups <= SFH_MAX_G && (2 * s->c) % s->groups == 0,
               "%s: groups=%d outside the supported 1..%d, or 2c=%d is no multiple of it", who, s->groups, SFH_MAX_G, 2 * s->c);
  MI_CHECK_ARG(s->H >= SFH_MIN_HW && s->W >= SFH_MIN_HW && s->H <= SFH_MAX_HW && s->W <= SFH_MAX_HW,
               "%s: H=%d W=%d outside the supported %d..%d (there is no fallback)", who, s->H, s->W, SFH_MIN_HW, SFH_MAX_HW);
  MI_CHECK_ARG(s->eps > 0.f && s->momentum >= 0.f && s->momentum <= 1.f, "%s: bad eps=%g or momentum=%g", who, (double)s->eps,
               (double)s->momentum);
  MI_CHECK_ARG(sfh_plan(s->B, s->c, s->groups, s->H, s->W, p), "%s: too many bins (B=%d c=%d H=%d W=%d)", who, s->B, s->c, s->H, s->W);
  return MI_OK;
}

// Z, (mu, r) -> t (SS_A), s (SS_S), ts (SS_B), W' (SS_WP), W' ts (SS_P): the forward's middle, run again by the backward
int sfh_middle(const SfhPlan& p, void* ws, const mi_fourier_unit_params* pr, const float* z, const float* stat, hipStream_t st) {
  const Sections<SFH_SECTIONS>& w = p.ws;
  const int bins = (int)p.bins;
  hipLaunchKernelGGL(sfh_fold_kernel, dim3(p.grid_w), dim3(SFH_THREADS), 0, st, pr->fdc_w, p.map, p.S, w.at(ws, SS_WP));
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_fpe_kernel, dim3(p.grid_elems), dim3(SFH_THREADS), 0, st, z, p.map, stat, pr->bn_w, pr->bn_b, pr->fpe_w,
                     pr->fpe_b, w.at(ws, SS_A), p.H, p.K, p.nblk);
  MI_LAUNCH_CHECK();
#define SFH_GATE(GG) launch_gate<GG>(dim3(p.grid_bins), st, (const float*)w.at(ws, SS_A), p.map, p.S, pr->gate_w, pr->gate_b, \
                                     w.at(ws, SS_S), w.at(ws, SS_B), p.N, bins)
  SFH_FOR_G(p.G, SFH_GATE)
#undef SFH_GATE
  MI_LAUNCH_CHECK();
  const mi_pw_desc d = conv1x1(w.at(ws, SS_B), p.C2, w.at(ws, SS_WP), false, p.C2, nullptr, nullptr, w.at(ws, SS_P), p.C2, p.B, p.N, MI_F32);
  return mi_pw_gemm(&d, w.at(ws, SS_PW), st);
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" size_t mi_fourier_unit_workspace(const mi_fourier_unit_shape* s) {
  SfhPlan p;
  return sfh_check("fourier_unit_workspace", s, &p) == MI_OK ? p.ws.total : 0;
}

extern "C" size_t mi_fourier_unit_saved_bytes(const mi_fourier_unit_shape* s) {
  SfhPlan p;
  return sfh_check("fourier_unit_saved_bytes", s, &p) == MI_OK ? p.saved.total : 0;
}

// The 17 scalars: planes B c, K, 2c, groups, channels per group, elements B 2c H K, bins B H K, threads per workgroup, bins per
// BatchNorm chunk, chunks per plane, partials per channel, grid of the per-element passes (1024 bins of one plane per workgroup),
// of the gate passes (64 bins per workgroup), own kernel launches forward / backward, library calls (1x1 product, Gram, channel
// sum) forward / backward.  The 18 SS_* sections from [18]; [62]: the offset of (mu, r) in the saved blob.  The format:
// plan_report, internal.h.
extern "C" int mi_fourier_unit_plan(const mi_fourier_unit_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "fourier_unit_plan: null pointer");
  SfhPlan p;
  MI_TRY(sfh_check("fourier_unit_plan", s, &p));
  return plan_report<18>(out, {(int64_t)p.B * p.c, p.K, p.C2, p.G, p.S, p.elems, p.bins, SFH_THREADS, SFH_CHUNK, p.nchunk, p.nparts,
                               p.grid_elems, p.grid_bins, p.kernels_fwd, p.kernels_bwd, p.lib_calls_fwd, p.lib_calls_bwd},
                         p.ws, {(int64_t)p.ws.total, (int64_t)p.saved.total, (int64_t)p.saved.off[1]});
}

extern "C" int mi_fourier_unit_fwd(const mi_fourier_unit_shape* s, const mi_fourier_unit_params* pr, const void* x, void* out,
                                   float* running_mean, float* running_var, void* saved, void* ws, void* stream) {
  SfhPlan p;
  MI_TRY(sfh_check("fourier_unit_fwd", s, &p));
  MI_CHECK_ARG(pr && pr->bn_w && pr->bn_b && pr->fdc_w && pr->fdc_b && pr->gate_w && pr->gate_b && pr->fpe_w && pr->fpe_b && x &&
               out && running_mean && running_var && ws, "fourier_unit_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<SFH_SECTIONS>& w = p.ws;
  const Dft2Ws dft = dft2_blob_ws(p.dft_blob, w.at(ws, SS_DFT));
  float* z = saved ? (float*)saved : w.at(ws, SS_Z);
  float* stat = saved ? p.saved.at(saved, 1) : w.at(ws, SS_STAT);
  float* o = w.at(ws, SS_U);
  const int64_t half = (int64_t)p.B * p.c * p.N;
  const double hw = (double)p.H * p.W;
  MI_TRY(dft2_tables(p.dft, dft, st));
  MI_TRY(dft2_r2c_run(p.dft, dft, x, z, z + half, s->dtype, st));
  if (s->training) {
    hipLaunchKernelGGL(bn_partial_kernel, dim3(p.nparts, p.C2), dim3(SFH_THREADS), 0, st, (const float*)z, p.map, p.N, p.nchunk,
                       w.at(ws, SS_BNP));
    MI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bn_finish_kernel, dim3(p.grid_chan), dim3(SFH_THREADS), 0, st, (const float*)w.at(ws, SS_BNP), p.map, p.N, p.nchunk,
                     p.nparts, (float)(1.0 / sqrt(hw)), s->eps, s->momentum, s->training, running_mean, running_var, stat);
  MI_LAUNCH_CHECK();
  MI_TRY(sfh_middle(p, ws, pr, z, stat, st));
  hipLaunchKernelGGL(sfh_gelu_kernel, dim3(p.grid_elems), dim3(SFH_THREADS), 0, st, (const float*)w.at(ws, SS_P),
                     (const float*)w.at(ws, SS_S), pr->fdc_b, p.map, p.G, o, (float)sqrt(hw), p.N, p.nblk);
  MI_LAUNCH_CHECK();
  return dft2_c2r_run(p.dft, dft, o, o + half, out, s->dtype, st);
}

extern "C" int mi_fourier_unit_bwd(const mi_fourier_unit_shape* s, const mi_fourier_unit_params* pr, const void* dout, void* dx,
                                   const mi_fourier_unit_grads* g, const void* saved, void* ws, void* stream) {
  SfhPlan p;
  MI_TRY(sfh_check("fourier_unit_bwd", s, &p));
  MI_CHECK_ARG(pr && pr->bn_w && pr->bn_b && pr->fdc_w && pr->fdc_b && pr->gate_w && pr->gate_b && pr->fpe_w && pr->fpe_b && dout &&
               dx && g && g->bn_w && g->bn_b && g->fdc_w && g->fdc_b && g->gate_w && g->gate_b && g->fpe_w && g->fpe_b && saved && ws,
               "fourier_unit_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<SFH_SECTIONS>& w = p.ws;
  const Dft2Ws dft = dft2_blob_ws(p.dft_blob, w.at(ws, SS_DFT));
  const int bins = (int)p.bins, acc = g->accumulate ? 1 : 0;
  const float* z = (const float*)saved;
  const float* stat = p.saved.at(saved, 1);
  float* u = w.at(ws, SS_U);
  const int64_t half = (int64_t)p.B * p.c * p.N;
  const double hw = (double)p.H * p.W;
  float* t = w.at(ws, SS_A); float* ts = w.at(ws, SS_B); float* dpre = w.at(ws, SS_P); float* q = w.at(ws, SS_Q);
  float* sg = w.at(ws, SS_S); float* dl = w.at(ws, SS_DL); float* tmp = w.at(ws, SS_GT); float* means = w.at(ws, SS_STAT) + 2 * p.C2;
  float* tmp_b = tmp + (size_t)p.C2 * p.C2; float* tmp_w = tmp_b + (size_t)p.G * p.C2;

  MI_TRY(dft2_tables(p.dft, dft, st));
  MI_TRY(dft2_c2r_adj(p.dft, dft, dout, u, u + half, s->dtype, st));    // H W x the adjoint
  MI_TRY(sfh_middle(p, ws, pr, z, stat, st));
  hipLaunchKernelGGL(sfh_gelu_bwd_kernel, dim3(p.grid_elems), dim3(SFH_THREADS), 0, st, dpre, (const float*)sg, pr->fdc_b, p.map, p.G,
                     (const float*)u, (float)(1.0 / sqrt(hw)), p.N, p.nblk);
  MI_LAUNCH_CHECK();
  MI_TRY(conv1x1_bwd_input(dpre, p.C2, ts, p.C2, w.at(ws, SS_WP), tmp, nullptr, q, p.B, p.N, MI_F32, 0, w.at(ws, SS_GRAM), w.at(ws, SS_CS),
                           w.at(ws, SS_PW), st, false));
  const mi_gram_desc gb = wgrad_gram(sg, p.G, dpre, p.C2, p.B, p.N, MI_F32, tmp_b, 0);
  MI_TRY(mi_gram(&gb, w.at(ws, SS_GRAM), st));
#define SFH_GATE_BWD(GG) launch_gate_bwd<GG>(dim3(p.grid_bins), st, (const float*)t, q, (const float*)dpre, (const float*)sg, p.map, \
                                             p.S, pr->gate_w, pr->fdc_b, dl, p.N, bins)
  SFH_FOR_G(p.G, SFH_GATE_BWD)
#undef SFH_GATE_BWD
  MI_LAUNCH_CHECK();
  const mi_gram_desc gw = wgrad_gram(dl, p.G, t, p.C2, p.B, p.N, MI_F32, tmp_w, 0);
  MI_TRY(mi_gram(&gw, w.at(ws, SS_GRAM), st));
  MI_TRY(launch_chan_sum(dl, g->gate_b, p.B, p.G, p.N, MI_F32, acc, w.at(ws, SS_CS), st));
  float* dt1 = ts;   // ts is dead: the Gram above was its last reader
  hipLaunchKernelGGL(fpe_bn_bwd_partial_kernel, dim3(p.nparts, p.C2), dim3(SFH_THREADS), 0, st, (const float*)q, z, p.map, stat,
                     pr->bn_w, pr->bn_b, pr->fpe_w, dt1, w.at(ws, SS_RP), p.H, p.K, p.nchunk);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(fpe_bn_bwd_finish_kernel, dim3(p.grid_fin), dim3(SFH_THREADS), 0, st, (const float*)w.at(ws, SS_RP), p.map, p.nparts,
                     (float)(1.0 / (double)p.bins), acc, g->fpe_w, g->fpe_b, g->bn_w, g->bn_b, means);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_bwd_dz_kernel, dim3(p.grid_elems), dim3(SFH_THREADS), 0, st, (const float*)dt1, z, p.map, stat,
                     (const float*)means, pr->bn_w, s->training, u, p.N, p.nblk);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(sfh_scatter_kernel, dim3(p.grid_scatter), dim3(SFH_THREADS), 0, st, (const float*)tmp, p.map, p.G, p.S, acc,
                     g->fdc_w, g->fdc_b, g->gate_w);
  MI_LAUNCH_CHECK();
  return dft2_r2c_adj(p.dft, dft, u, u + half, dx, s->dtype, st);
}
