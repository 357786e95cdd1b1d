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
// The stages are dft2.hip's (dft2.h): its GEMM kernel, its table fill, its tile and grid geometry.  fl_plan adds what is the
// loss's own, the workspace sections, the partial count and the number of launches: mi_fft_l1_loss launches what it says,
// mi_fft_l1_workspace sizes from it, mi_fft_l1_plan reports it.
#include "dft2.h"

namespace mi {
namespace {

constexpr int FL_SECTIONS = 10;

struct FlPlan {
  Dft2Geom g;                        // tiles and grids of the four stages and of the table fill
  int grid3, grid4;                  // stages 3 and 4 as launched (0 without the gradient)
  int partials, reduce_launches, launches;
  bool want_grad;
  // cos W | sin W [W][K], their transposes [K][W], cos H | sin H [H][H], T (re | im, [P*H][K] each; gT reuses it),
  // S (the same shape), the loss partials, the two-stage sum's scratch
  size_t off[FL_SECTIONS], bytes[FL_SECTIONS], total;
};
enum { SEC_CW = 0, SEC_SW, SEC_CWT, SEC_SWT, SEC_CH, SEC_SH, SEC_T, SEC_S, SEC_PART, SEC_RED };

bool fl_plan(int B, int C, int H, int W, bool want_grad, FlPlan* p) {
  *p = FlPlan{};
  if (B <= 0 || C <= 0 || !dft2_geom((int64_t)B * C, H, W, &p->g)) return false;
  const Dft2Geom& g = p->g;
  p->want_grad = want_grad;
  p->grid3 = want_grad ? g.grid_plane : 0; p->grid4 = want_grad ? g.grid_fold_x : 0;
  p->partials = g.grid_plane;
  p->reduce_launches = reduce_rows_two_stage(p->partials) ? 2 : 1;
  p->launches = 3 + p->reduce_launches + (want_grad ? 2 : 0);
  const size_t wk = dft2_table_bytes(g, DT_CW), hh = dft2_table_bytes(g, DT_CH), t = (size_t)g.P * H * g.K * 2 * 4;
  const size_t sz[FL_SECTIONS] = {wk, wk, wk, wk, hh, hh, t, t, (size_t)p->partials * 4, (size_t)REDUCE_GROUPS * 4};
  size_t o = 0;
  for (int i = 0; i < FL_SECTIONS; ++i) { p->off[i] = o; p->bytes[i] = sz[i]; o = align_up(o + sz[i], 256); }
  p->total = o;
  return true;
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
  const Dft2Geom& g = p.g;
  int64_t v[40] = {g.P, g.K, FL_TM, FL_KC, 16 * g.nf_l, g.l_blocks, 16 * g.nf_x, g.x_blocks, g.m_tiles_fold, g.m_tiles_plane,
                   g.grid_tab, g.grid_fold_l, g.grid_plane, p.grid3, p.grid4, FL_THREADS, p.partials, p.reduce_launches, p.launches};
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
  const int64_t bins = (int64_t)p.g.P * H * p.g.K;
  Dft2Ws w = {};   // no weighted tables: the loss launches the stages, never c2r
  w.tab[DT_CW] = sec(SEC_CW); w.tab[DT_SW] = sec(SEC_SW); w.tab[DT_CWT] = sec(SEC_CWT); w.tab[DT_SWT] = sec(SEC_SWT);
  w.tab[DT_CH] = sec(SEC_CH); w.tab[DT_SH] = sec(SEC_SH);
  w.tre = sec(SEC_T); w.tim = w.tre + bins;
  float* sre = p.want_grad ? sec(SEC_S) : nullptr; float* sim = p.want_grad ? sre + bins : nullptr;
  const float scale = (float)((double)loss_weight / (2.0 * (double)bins));

  MI_TRY(dft2_tables(p.g, w, st));
  MI_TRY(dft2_rows_fwd(p.g, pred, target, w.tab[DT_CW], w.tab[DT_SW], w.tre, w.tim, dtype, st));   // T = d . E_W
  MI_TRY(dft2_cols_sign(p.g, w, w.tre, w.tim, sre, sim, sec(SEC_PART), st));                       // Z = E_H . T -> S, partials
  MI_TRY(launch_reduce_rows(sec(SEC_PART), loss, p.partials, 1, 1, 0, scale, st, sec(SEC_RED)));
  if (!p.want_grad) return MI_OK;
  MI_TRY(dft2_cols(p.g, w, 1.f, sre, sim, w.tre, w.tim, st));                                      // gT = conj(E_H) . S, into T
  return dft2_rows_bwd(p.g, w.tre, w.tim, w.tab[DT_CWT], w.tab[DT_SWT], dpred, scale, dtype, st);  // dpred = scale Re(gT . conj(E_W)^T)
}
