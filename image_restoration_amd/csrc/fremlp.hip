// DarkIR's FreMLP (DarkIR-main/archs/arch_model.py:36-55) and the two real 2-D transforms it stands on, without an FFT library:
// the dense-DFT GEMMs of dft2.hip (dft2.h: exact fp32-input MFMA, exact quarter-turn twiddles), fp32 between the input load
// and the output store.
//
//   K = W/2 + 1,  P = B*nc planes,  hc = expand*nc,  E_N[a][b] = exp(-2 pi i ((a b) mod N) / N)
//   r2c   T = x . E_W  (planes folded into the rows);   Z = E_H . T per plane                          = rfft2(x)
//   polar mag = sqrt(Re Z^2 + Im Z^2),  u = Z / mag,  u = (1, 0) where mag == 0   (no atan2, cos or sin)
//   MLP   a = LeakyReLU_0.1(W1 mag + b1),  mag' = W2 a + b2   over channels, per frequency bin (mi_pw_gemm at fp32)
//   c2r   Y = mag' u;   V = conj(E_H) . Y per plane;   out = 1/(HW) Re(V . Bt),  Bt[l][x] = w_l exp(+2 pi i l x / W),
//         w_l = 1 at l = 0 and (even W) l = W/2, else 2                                                = irfft2(Y, s=(H, W))
// Backward: GV = dout . conj(Bt)^T;  G = 1/(HW) E_H . GV  (the adjoint of c2r);  dmag' = G . u,  du = mag' G;  the MLP backward
// (mi_gram, the channel sum, W^T dY) gives dmag and the parameter gradients;  dZ = dmag u + (du - u (u . du)) / mag, 0 where
// mag == 0;  dx = Re(conj(E_H) . dZ . conj(E_W)^T)  (the adjoint of r2c: stages 3 and 4 of the FFT loss).
// Saved for the backward: Z and a (fp32); mag, u and mag' are recomputed from them.
// The transforms' tiles and grids are dft2_geom's.  fre_plan adds what is FreMLP's own, the grids of the per-bin passes, the
// workspace sections and the launch counts: the launchers launch what it says, mi_fremlp_workspace / mi_fremlp_saved_bytes size
// from it, mi_fremlp_plan reports it.
#include <limits.h>

#include "dft2.h"

namespace mi {
namespace {

constexpr int FRE_MAX_NC = 256, FRE_MAX_HC = 512;
constexpr float FRE_SLOPE = 0.1f;
// The transforms' blob (dft2.h: the ten DT_* tables, then T, its complex [P*H][K] intermediate); U: a second complex [P*H][K]
// (re | im); Z and A: the saved blob's two parts when the caller keeps none (A also holds the hidden gradient in the backward);
// M1, M2: two real [P*H][K] planes; the three library workspaces.
enum { FS_T = DFT2_TABLES, FS_U, FS_Z, FS_A, FS_M1, FS_M2, FS_PW, FS_GRAM, FS_CS, FRE_SECTIONS };

struct FrePlan {
  int B, nc, hc;
  Dft2Geom g;                                           // the transforms' tiles and grids
  Dft2Blob dft;                                         // ... and their blob, which opens the workspace
  int grid_bins, grid_hidden;                           // elementwise passes over P*H*K bins / over B*hc*H*K hidden values
  int kernels_fwd, kernels_bwd, lib_calls_fwd, lib_calls_bwd;   // own launches; mi_pw_gemm / mi_gram / channel-sum calls
  int64_t bins, hidden;
  Sections<FRE_SECTIONS> ws;
  Sections<2> saved;                                    // the blob: Z (re | im), then a
};

bool fre_plan(int B, int nc, int expand, int H, int W, FrePlan* p) {
  *p = FrePlan{};
  if (B <= 0 || nc <= 0 || expand <= 0 || nc > FRE_MAX_NC || (int64_t)expand * nc > FRE_MAX_HC) return false;
  if (!dft2_geom((int64_t)B * nc, H, W, &p->g) || !dft2_blob(p->g, &p->dft)) return false;
  const int K = p->g.K, hc = expand * nc;
  const int64_t bins = p->dft.bins, hidden = (int64_t)B * hc * H * K, N = (int64_t)H * K;
  if (hidden > INT_MAX) return false;
  p->B = B; p->nc = nc; p->hc = hc;
  p->bins = bins; p->hidden = hidden;
  p->grid_bins = cdiv(bins, FL_THREADS); p->grid_hidden = cdiv(hidden, FL_THREADS);
  // forward: tables, r2c (2), |Z|, LeakyReLU, Y = mag' u, c2r (2); two 1x1 products
  // backward: tables, GV, G, (dmag', du), LeakyReLU', |Z|, dZ, the r2c adjoint (2); mag' again, and per 1x1 conv a Gram, a
  // channel sum and W^T dY
  p->kernels_fwd = 8; p->kernels_bwd = 9; p->lib_calls_fwd = 2; p->lib_calls_bwd = 7;
  const size_t cplx = (size_t)bins * 2 * 4, real = (size_t)bins * 4;
  Sections<FRE_SECTIONS>& ws = p->ws;
  for (int i = 0; i < DFT2_TABLES; ++i) ws.place(i, p->dft.tab[i], dft2_table_bytes(p->g, i));
  ws.place(FS_T, p->dft.t, cplx);
  ws.total = p->dft.total;   // FreMLP's own sections follow the transforms' blob
  ws.put(FS_U, cplx); ws.put(FS_Z, cplx); ws.put(FS_A, (size_t)hidden * 4); ws.put(FS_M1, real); ws.put(FS_M2, real);
  ws.put(FS_PW, max_of({pw_ws_bytes(probe1x1(nc, hc, false, B, N, MI_F32)), pw_ws_bytes(probe1x1(hc, nc, false, B, N, MI_F32)),
                        pw_ws_bytes(probe1x1(nc, hc, true, B, N, MI_F32)), pw_ws_bytes(probe1x1(hc, nc, true, B, N, MI_F32))}));
  ws.put(FS_GRAM, max_of({gram_ws_bytes(probe_wgrad(nc, hc, B, N, MI_F32)), gram_ws_bytes(probe_wgrad(hc, nc, B, N, MI_F32))}));
  ws.put(FS_CS, max_of({chan_sum_workspace(hc, N), chan_sum_workspace(nc, N)}));
  p->saved.put(0, cplx); p->saved.put(1, (size_t)hidden * 4);
  return true;
}

// The polar form of one bin, the same arithmetic wherever it is (re)computed.  mag == 0 (both parts zero, or so small that their
// squares vanish): u = (1, 0), as torch.angle(0) = 0.
__device__ __forceinline__ void fre_polar(float re, float im, float* mag, float* ur, float* ui) {
  const float m = sqrtf(re * re + im * im);
  *mag = m;
  if (m > 0.f) { *ur = re / m; *ui = im / m; } else { *ur = 1.f; *ui = 0.f; }
}

__global__ __launch_bounds__(FL_THREADS) void fre_mag_kernel(const float* __restrict__ zre, const float* __restrict__ zim,
                                                             float* __restrict__ mag, int n) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= n) return;
  float m, ur, ui;
  fre_polar(zre[i], zim[i], &m, &ur, &ui);
  mag[i] = m;
}

// a = LeakyReLU(h) in place (BWD: da *= LeakyReLU'(h), read off the sign of the stored a: a > 0 exactly where h > 0)
template <bool BWD>
__global__ __launch_bounds__(FL_THREADS) void fre_leaky_kernel(float* __restrict__ h, const float* __restrict__ a, int n) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= n) return;
  const float v = h[i];
  if (BWD) h[i] = a[i] > 0.f ? v : FRE_SLOPE * v;
  else h[i] = v > 0.f ? v : FRE_SLOPE * v;
}

// Y = mag' u
__global__ __launch_bounds__(FL_THREADS) void fre_compose_kernel(const float* __restrict__ zre, const float* __restrict__ zim,
                                                                 const float* __restrict__ mag2, float* __restrict__ yre,
                                                                 float* __restrict__ yim, int n) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= n) return;
  float m, ur, ui;
  fre_polar(zre[i], zim[i], &m, &ur, &ui);
  const float v = mag2[i];
  yre[i] = v * ur; yim[i] = v * ui;
}

// G = scale * (the stored product);  dmag' = G . u;  du = mag' G, over G in place
__global__ __launch_bounds__(FL_THREADS) void fre_bwd_g_kernel(const float* __restrict__ zre, const float* __restrict__ zim,
                                                               const float* __restrict__ mag2, float* __restrict__ gre,
                                                               float* __restrict__ gim, float* __restrict__ dmag2, float scale,
                                                               int n) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= n) return;
  float m, ur, ui;
  fre_polar(zre[i], zim[i], &m, &ur, &ui);
  const float gr = scale * gre[i], gi = scale * gim[i], v = mag2[i];
  dmag2[i] = gr * ur + gi * ui;
  gre[i] = v * gr; gim[i] = v * gi;
}

// dZ = dmag u + (du - u (u . du)) / mag, over du in place; 0 where mag == 0 (abs and angle have zero gradient there)
__global__ __launch_bounds__(FL_THREADS) void fre_bwd_dz_kernel(const float* __restrict__ zre, const float* __restrict__ zim,
                                                                const float* __restrict__ dmag, float* __restrict__ dre,
                                                                float* __restrict__ dim, int n) {
  const int i = blockIdx.x * FL_THREADS + threadIdx.x;
  if (i >= n) return;
  float m, ur, ui;
  fre_polar(zre[i], zim[i], &m, &ur, &ui);
  float or_ = 0.f, oi = 0.f;
  if (m > 0.f) {
    const float dr = dre[i], di = dim[i], dm = dmag[i];
    const float dot = ur * dr + ui * di;
    or_ = dm * ur + (dr - ur * dot) / m;
    oi = dm * ui + (di - ui * dot) / m;
  }
  dre[i] = or_; dim[i] = oi;
}

int fre_check(const char* who, const mi_fremlp_shape* s, FrePlan* p) {
  MI_CHECK_ARG(s, "%s: null shape", who);
  MI_CHECK_ARG(s->dtype == MI_F32 || s->dtype == MI_BF16, "%s: bad dtype %d", who, s->dtype);
  MI_CHECK_ARG(s->B > 0, "%s: bad shape B=%d", who, s->B);
  MI_CHECK_ARG(s->nc >= 1 && s->nc <= FRE_MAX_NC && s->expand >= 1 && (int64_t)s->expand * s->nc <= FRE_MAX_HC,
               "%s: nc=%d expand=%d outside the supported 1 <= nc <= %d, expand >= 1, expand*nc <= %d", who, s->nc, s->expand,
               FRE_MAX_NC, FRE_MAX_HC);
  MI_CHECK_ARG(s->H >= FL_MIN && s->W >= FL_MIN && s->H <= FL_MAX && s->W <= FL_MAX,
               "%s: H=%d W=%d outside the supported %d..%d (there is no fallback)", who, s->H, s->W, FL_MIN, FL_MAX);
  MI_CHECK_ARG(fre_plan(s->B, s->nc, s->expand, s->H, s->W, p), "%s: too many bins (B=%d nc=%d expand=%d H=%d W=%d)", who, s->B,
               s->nc, s->expand, s->H, s->W);
  return MI_OK;
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" size_t mi_fremlp_workspace(const mi_fremlp_shape* s) {
  FrePlan p;
  return fre_check("fremlp_workspace", s, &p) == MI_OK ? p.ws.total : 0;
}

extern "C" size_t mi_fremlp_saved_bytes(const mi_fremlp_shape* s) {
  FrePlan p;
  return fre_check("fremlp_saved_bytes", s, &p) == MI_OK ? p.saved.total : 0;
}

// The 22 scalars: planes P, K = W/2 + 1, hidden width, tile rows (64), contraction depth per LDS stage (16), l block width, l
// blocks, x block width, x blocks, 64-row tiles over P*H, 64-row tiles over H, grid of the table fill, of the [P*H] x K stages, of
// the per-plane stages, of the [P*H] x W stages, of the per-bin passes, of the hidden passes, threads per workgroup, own kernel
// launches forward / backward, library calls (1x1 product, Gram, channel sum) forward / backward.  The 19 sections (the ten DT_*
// tables, then the FS_* list) from [22]; [62]: the offset of `a` in the saved blob.  The format: plan_report, internal.h.
extern "C" int mi_fremlp_plan(const mi_fremlp_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "fremlp_plan: null pointer");
  FrePlan p;
  MI_TRY(fre_check("fremlp_plan", s, &p));
  const Dft2Geom& g = p.g;
  return plan_report<22>(out, {g.P, g.K, p.hc, FL_TM, FL_KC, 16 * g.nf_l, g.l_blocks, 16 * g.nf_x, g.x_blocks, g.m_tiles_fold,
                               g.m_tiles_plane, g.grid_tab, g.grid_fold_l, g.grid_plane, g.grid_fold_x, p.grid_bins, p.grid_hidden,
                               FL_THREADS, p.kernels_fwd, p.kernels_bwd, p.lib_calls_fwd, p.lib_calls_bwd},
                         p.ws, {(int64_t)p.ws.total, (int64_t)p.saved.total, (int64_t)p.saved.off[1]});
}

extern "C" int mi_fremlp_fwd(const mi_fremlp_shape* s, const float* w1, const float* b1, const float* w2, const float* b2,
                             const void* x, void* out, void* saved, void* ws, void* stream) {
  FrePlan p;
  MI_TRY(fre_check("fremlp_fwd", s, &p));
  MI_CHECK_ARG(w1 && b1 && w2 && b2 && x && out && ws, "fremlp_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<FRE_SECTIONS>& w = p.ws;
  const Dft2Ws dft = dft2_blob_ws(p.dft, ws);   // the tables and T
  const int n = (int)p.bins, nh = (int)p.hidden;
  const int64_t N = (int64_t)p.g.H * p.g.K;
  float* ure = w.at(ws, FS_U); float* uim = ure + n;
  float* zre = saved ? (float*)saved : w.at(ws, FS_Z); float* zim = zre + n;
  float* a = saved ? p.saved.at(saved, 1) : w.at(ws, FS_A);
  float* mag = w.at(ws, FS_M1); float* mag2 = w.at(ws, FS_M2);

  MI_TRY(dft2_tables(p.g, dft, st));
  MI_TRY(dft2_r2c_run(p.g, dft, x, zre, zim, s->dtype, st));
  hipLaunchKernelGGL(fre_mag_kernel, dim3(p.grid_bins), dim3(FL_THREADS), 0, st, zre, zim, mag, n);
  MI_LAUNCH_CHECK();
  const mi_pw_desc d1 = conv1x1(mag, p.nc, w1, false, p.nc, b1, nullptr, a, p.hc, p.B, N, MI_F32);
  MI_TRY(mi_pw_gemm(&d1, w.at(ws, FS_PW), stream));
  hipLaunchKernelGGL(fre_leaky_kernel<false>, dim3(p.grid_hidden), dim3(FL_THREADS), 0, st, a, (const float*)nullptr, nh);
  MI_LAUNCH_CHECK();
  const mi_pw_desc d2 = conv1x1(a, p.hc, w2, false, p.hc, b2, nullptr, mag2, p.nc, p.B, N, MI_F32);
  MI_TRY(mi_pw_gemm(&d2, w.at(ws, FS_PW), stream));
  hipLaunchKernelGGL(fre_compose_kernel, dim3(p.grid_bins), dim3(FL_THREADS), 0, st, zre, zim, mag2, dft.tre, dft.tim, n);
  MI_LAUNCH_CHECK();
  Dft2Ws via = dft;   // Y sits in T, which r2c is done with, so c2r passes through U
  via.tre = ure; via.tim = uim;
  return dft2_c2r_run(p.g, via, dft.tre, dft.tim, out, s->dtype, st);
}

extern "C" int mi_fremlp_bwd(const mi_fremlp_shape* s, const float* w1, const float* w2, const float* b2, const void* dout,
                             void* dx, float* g_w1, float* g_b1, float* g_w2, float* g_b2, int accumulate, const void* saved,
                             void* ws, void* stream) {
  FrePlan p;
  MI_TRY(fre_check("fremlp_bwd", s, &p));
  MI_CHECK_ARG(w1 && w2 && b2 && dout && dx && g_w1 && g_b1 && g_w2 && g_b2 && saved && ws, "fremlp_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Sections<FRE_SECTIONS>& w = p.ws;
  const Dft2Ws dft = dft2_blob_ws(p.dft, ws);   // the tables and T
  const int n = (int)p.bins, nh = (int)p.hidden;
  const int64_t N = (int64_t)p.g.H * p.g.K;
  float* ure = w.at(ws, FS_U); float* uim = ure + n;
  const float* zre = (const float*)saved; const float* zim = zre + n;
  const float* a = p.saved.at(saved, 1);
  float* da = w.at(ws, FS_A); float* m1 = w.at(ws, FS_M1); float* m2 = w.at(ws, FS_M2);

  MI_TRY(dft2_tables(p.g, dft, st));
  MI_TRY(dft2_c2r_adj(p.g, dft, dout, ure, uim, s->dtype, st));                             // G (unscaled), through GV
  const mi_pw_desc d2 = conv1x1(a, p.hc, w2, false, p.hc, b2, nullptr, m2, p.nc, p.B, N, MI_F32);   // mag' again
  MI_TRY(mi_pw_gemm(&d2, w.at(ws, FS_PW), stream));
  hipLaunchKernelGGL(fre_bwd_g_kernel, dim3(p.grid_bins), dim3(FL_THREADS), 0, st, zre, zim, (const float*)m2, ure, uim, m1,
                     (float)(1.0 / ((double)p.g.H * p.g.W)), n);                                 // m1 = dmag', U = du
  MI_LAUNCH_CHECK();
  MI_TRY(conv1x1_bwd_input(m1, p.nc, a, p.hc, w2, g_w2, g_b2, da, p.B, N, MI_F32, accumulate, w.at(ws, FS_GRAM), w.at(ws, FS_CS),
                           w.at(ws, FS_PW), st, false));
  hipLaunchKernelGGL(fre_leaky_kernel<true>, dim3(p.grid_hidden), dim3(FL_THREADS), 0, st, da, a, nh);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(fre_mag_kernel, dim3(p.grid_bins), dim3(FL_THREADS), 0, st, zre, zim, m2, n);   // m2 = mag
  MI_LAUNCH_CHECK();
  MI_TRY(conv1x1_bwd_input(da, p.hc, m2, p.nc, w1, g_w1, g_b1, m1, p.B, N, MI_F32, accumulate, w.at(ws, FS_GRAM), w.at(ws, FS_CS),
                           w.at(ws, FS_PW), st, false));                                        // m1 = dmag
  hipLaunchKernelGGL(fre_bwd_dz_kernel, dim3(p.grid_bins), dim3(FL_THREADS), 0, st, zre, zim, (const float*)m1, ure, uim, n);
  MI_LAUNCH_CHECK();
  return dft2_r2c_adj(p.g, dft, ure, uim, dx, s->dtype, st);
}
