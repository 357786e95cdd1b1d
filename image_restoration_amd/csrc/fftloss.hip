// FFT loss (MoCE-IR-main/src/utils/loss_utils.py:139-152): loss_weight * mean(|Re| + |Im|) of rfft2(pred - target), and its
// gradient, as four dense-DFT GEMMs on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32).  No FFT library, no atomics, no
// state: twiddle tables, intermediates and the loss partials live in the caller's workspace and are rebuilt each call.
//
//   d = pred - target (widened to fp32 on load),  K = W/2 + 1,  P = B*C planes
//   stage 1   T  = d . E_W          [P*H x W] real  x [W x K] complex      (planes folded into the rows: E_W is shared)
//   stage 2   Z  = E_H . T          [H x H] complex x [H x K] complex per plane; Z is never stored: the epilogue writes
//                                   S = sign(Re Z) + i sign(Im Z) and one |Re| + |Im| partial per workgroup
//   (reduce)  loss = loss_weight / (2 P H K) * sum of the partials, in a fixed order
//   stage 3   gT = conj(E_H) . S    the same kernel with the sine table's sign flipped
//   stage 4   dpred = scale * Re(gT . conj(E_W)^T)   [P*H x K] complex x [K x W] complex, real part only, rounded once
// E_N[a][b] = exp(-2 pi i ((a b) mod N) / N).  With dpred == NULL stages 3 and 4 (and the S stores) are skipped.
// One kernel template serves the four stages; fl_plan is the ONE place that decides tiles, grids, workspace sections and the
// number of launches: mi_fft_l1_loss launches what it says, mi_fft_l1_workspace sizes from it, mi_fft_l1_plan reports it.
#include <limits.h>

#include "fl_gemm.h"   // the GEMM kernel template, the twiddle and tile-width rules (shared with fremlp.hip)

namespace mi {
namespace {

constexpr int FL_SECTIONS = 10;

struct FlPlan {
  int P, H, W, K;
  int nf_l, nf_x;                    // 16-column fragments per tile over l (stages 1-3) and over x (stage 4): 3, 4 or 5
  int l_blocks, x_blocks;            // tiles over K and over W
  int m_tiles_fold, m_tiles_plane;   // 64-row tiles over P*H (stages 1, 4) and over H (stages 2, 3: one set per plane)
  int grid_tab, grid1, grid2, grid3, grid4;
  int partials, reduce_launches, launches;
  bool want_grad;
  // cos W | sin W [W][K], their transposes [K][W], cos H | sin H [H][H], T (re | im, [P*H][K] each; gT reuses it),
  // S (the same shape), the loss partials, the two-stage sum's scratch
  size_t off[FL_SECTIONS], bytes[FL_SECTIONS], total;
};
enum { SEC_CW = 0, SEC_SW, SEC_CWT, SEC_SWT, SEC_CH, SEC_SH, SEC_T, SEC_S, SEC_PART, SEC_RED };

bool fl_plan(int B, int C, int H, int W, bool want_grad, FlPlan* p) {
  *p = FlPlan{};
  if (B <= 0 || C <= 0 || H < FL_MIN || W < FL_MIN || H > FL_MAX || W > FL_MAX) return false;
  const int64_t P = (int64_t)B * C;
  if (P * H > (1 << 30)) return false;
  p->P = (int)P; p->H = H; p->W = W; p->K = W / 2 + 1;
  p->want_grad = want_grad;
  const int K = p->K;
  p->nf_l = fl_pick_nf(K); p->nf_x = fl_pick_nf(W);
  p->l_blocks = cdiv(K, 16 * p->nf_l); p->x_blocks = cdiv(W, 16 * p->nf_x);
  p->m_tiles_fold = cdiv(P * H, FL_TM); p->m_tiles_plane = cdiv(H, FL_TM);
  const int64_t g1 = (int64_t)p->m_tiles_fold * p->l_blocks, g2 = P * p->m_tiles_plane * p->l_blocks,
                g4 = (int64_t)p->m_tiles_fold * p->x_blocks;
  if (g1 > INT_MAX || g2 > INT_MAX || g4 > INT_MAX) return false;
  p->grid_tab = cdiv((int64_t)W * K + (int64_t)H * H, FL_THREADS);
  p->grid1 = (int)g1; p->grid2 = (int)g2;
  p->grid3 = want_grad ? (int)g2 : 0; p->grid4 = want_grad ? (int)g4 : 0;
  p->partials = p->grid2;
  p->reduce_launches = reduce_rows_two_stage(p->partials) ? 2 : 1;
  p->launches = 3 + p->reduce_launches + (want_grad ? 2 : 0);
  const size_t wk = (size_t)W * K * 4, hh = (size_t)H * H * 4, t = (size_t)P * H * K * 2 * 4;
  const size_t sz[FL_SECTIONS] = {wk, wk, wk, wk, hh, hh, t, t, (size_t)p->partials * 4, (size_t)REDUCE_GROUPS * 4};
  size_t o = 0;
  for (int i = 0; i < FL_SECTIONS; ++i) { p->off[i] = o; p->bytes[i] = sz[i]; o = align_up(o + sz[i], 256); }
  p->total = o;
  return true;
}

__global__ __launch_bounds__(FL_THREADS) void fl_tables_kernel(float* __restrict__ cw, float* __restrict__ sw,
                                                               float* __restrict__ cwt, float* __restrict__ swt,
                                                               float* __restrict__ ch, float* __restrict__ sh, int H, int W,
                                                               int K) {
  const int idx = blockIdx.x * FL_THREADS + threadIdx.x;
  float c, s;
  if (idx < W * K) {
    const int x = idx / K, l = idx - x * K;
    fl_twiddle((x * l) % W, W, &c, &s);
    cw[idx] = c; sw[idx] = s;
    cwt[l * W + x] = c; swt[l * W + x] = s;
  } else if (idx < W * K + H * H) {
    const int j = idx - W * K;
    const int k = j / H, y = j - k * H;
    fl_twiddle((k * y) % H, H, &c, &s);
    ch[j] = c; sh[j] = s;
  }
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" size_t mi_fft_l1_workspace(int B, int C, int H, int W) {
  FlPlan p;
  return fl_plan(B, C, H, W, true, &p) ? p.total : 0;
}

// out[40]: planes P, K = W/2 + 1, tile rows (64), contraction depth per LDS stage (16), l block width, l blocks, x block width,
// x blocks, 64-row tiles over P*H, 64-row tiles over H, grid of the table fill, of stages 1..4 (0: not launched), threads per
// workgroup, loss partials, launches of their sum, launches in all; then (byte offset, bytes) of the ten workspace sections
// cos W, sin W, cos W^T, sin W^T, cos H, sin H, T (gT reuses it), S, partials, the sum's scratch; last, the workspace size.
extern "C" int mi_fft_l1_plan(int B, int C, int H, int W, int dtype, int want_grad, int64_t* out) {
  MI_CHECK_ARG(out, "fft_l1_plan: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "fft_l1_plan: bad dtype %d", dtype);
  MI_CHECK_ARG(B > 0 && C > 0, "fft_l1_plan: bad shape B=%d C=%d", B, C);
  MI_CHECK_ARG(H >= FL_MIN && W >= FL_MIN && H <= FL_MAX && W <= FL_MAX,
               "fft_l1_plan: H=%d W=%d outside the supported %d..%d (there is no fallback)", H, W, FL_MIN, FL_MAX);
  FlPlan p;
  MI_CHECK_ARG(fl_plan(B, C, H, W, want_grad != 0, &p), "fft_l1_plan: too many planes (B=%d C=%d H=%d)", B, C, H);
  int64_t v[40] = {p.P, p.K, FL_TM, FL_KC, 16 * p.nf_l, p.l_blocks, 16 * p.nf_x, p.x_blocks, p.m_tiles_fold, p.m_tiles_plane,
                   p.grid_tab, p.grid1, p.grid2, p.grid3, p.grid4, FL_THREADS, p.partials, p.reduce_launches, p.launches};
  for (int i = 0; i < FL_SECTIONS; ++i) { v[19 + 2 * i] = (int64_t)p.off[i]; v[20 + 2 * i] = (int64_t)p.bytes[i]; }
  v[39] = (int64_t)p.total;
  memcpy(out, v, sizeof(v));
  return MI_OK;
}

extern "C" int mi_fft_l1_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                              float loss_weight, int dtype, void* ws, void* stream) {
  MI_CHECK_ARG(pred && target && loss && ws, "fft_l1_loss: null pointer");
  MI_CHECK_ARG(dtype == MI_F32 || dtype == MI_BF16, "fft_l1_loss: bad dtype %d", dtype);
  MI_CHECK_ARG(B > 0 && C > 0, "fft_l1_loss: bad shape B=%d C=%d", B, C);
  MI_CHECK_ARG(H >= FL_MIN && W >= FL_MIN && H <= FL_MAX && W <= FL_MAX,
               "fft_l1_loss: H=%d W=%d outside the supported %d..%d (there is no fallback)", H, W, FL_MIN, FL_MAX);
  FlPlan p;
  MI_CHECK_ARG(fl_plan(B, C, H, W, dpred != nullptr, &p), "fft_l1_loss: too many planes (B=%d C=%d H=%d)", B, C, H);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  auto sec = [&](int i) { return (float*)(base + p.off[i]); };
  const int K = p.K;
  const int64_t PH = (int64_t)p.P * H, plane = (int64_t)H * K;
  float* tre = sec(SEC_T); float* tim = tre + PH * K;
  float* sre = sec(SEC_S); float* sim = sre + PH * K;
  const float scale = (float)((double)loss_weight / (2.0 * (double)PH * K));

  hipLaunchKernelGGL(fl_tables_kernel, dim3(p.grid_tab), dim3(FL_THREADS), 0, st, sec(SEC_CW), sec(SEC_SW), sec(SEC_CWT),
                     sec(SEC_SWT), sec(SEC_CH), sec(SEC_SH), H, W, K);
  MI_LAUNCH_CHECK();

  FlGemm g1 = {};   // T = d . E_W
  g1.a0 = pred; g1.a1 = target; g1.lda = W;
  g1.b0 = sec(SEC_CW); g1.b1 = sec(SEC_SW); g1.ldb = K; g1.b_sign = -1.f;
  g1.c0 = tre; g1.c1 = tim; g1.ldc = K;
  g1.M = (int)PH; g1.N = K; g1.Kd = W; g1.m_tiles = p.m_tiles_fold; g1.n_tiles = p.l_blocks;
  MI_TRY(with_dtype(dtype, "fft_l1_loss", [&](auto tag) -> int {
    return fl_launch<A_DIFF, E_CPLX, decltype(tag)>(p.nf_l, g1, p.grid1, st);
  }));

  FlGemm g2 = {};   // Z = E_H . T per plane -> S, partials
  g2.a0 = sec(SEC_CH); g2.a1 = sec(SEC_SH); g2.lda = H; g2.a_sign = -1.f;
  g2.b0 = tre; g2.b1 = tim; g2.ldb = K; g2.b_zs = plane; g2.b_sign = 1.f;
  g2.c0 = p.want_grad ? sre : nullptr; g2.c1 = p.want_grad ? sim : nullptr; g2.ldc = K; g2.c_zs = plane;
  g2.part = sec(SEC_PART);
  g2.M = H; g2.N = K; g2.Kd = H; g2.m_tiles = p.m_tiles_plane; g2.n_tiles = p.l_blocks;
  MI_TRY((fl_launch<A_CPLX, E_SIGN, float>(p.nf_l, g2, p.grid2, st)));
  MI_TRY(launch_reduce_rows(sec(SEC_PART), loss, p.partials, 1, 1, 0, scale, st, sec(SEC_RED)));
  if (!p.want_grad) return MI_OK;

  FlGemm g3 = g2;   // gT = conj(E_H) . S per plane, into T's section
  g3.a_sign = 1.f;
  g3.b0 = sre; g3.b1 = sim;
  g3.c0 = tre; g3.c1 = tim; g3.part = nullptr;
  MI_TRY((fl_launch<A_CPLX, E_CPLX, float>(p.nf_l, g3, p.grid3, st)));

  FlGemm g4 = {};   // dpred = scale * Re(gT . conj(E_W)^T)
  g4.a0 = tre; g4.a1 = tim; g4.lda = K; g4.a_sign = 1.f;
  g4.b0 = sec(SEC_CWT); g4.b1 = sec(SEC_SWT); g4.ldb = W; g4.b_sign = 1.f;
  g4.c0 = dpred; g4.ldc = W; g4.scale = scale;
  g4.M = (int)PH; g4.N = W; g4.Kd = K; g4.m_tiles = p.m_tiles_fold; g4.n_tiles = p.x_blocks;
  return with_dtype(dtype, "fft_l1_loss", [&](auto tag) -> int {
    return fl_launch<A_CPLX, E_REAL, decltype(tag)>(p.nf_x, g4, p.grid4, st);
  });
}
