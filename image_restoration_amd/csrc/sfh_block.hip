// SFHformer's Block (SFHformer.py:254-282) as one launch sequence forward and one backward.  No kernel and no arithmetic of its own:
// host code that calls mi_bn2d_*, mi_scale_res_*, mi_sfh_mixer_* and mi_sfh_ffn_* on sections of its own buffers, so every launch
// goes through a launcher whose argument checks and kernels are covered where that launcher lives.
//   forward   y1 = norm1(x; part_in)          m = Mixer(y1)      x1 = m beta + x      (training: with the pairs p1 of x1)
//             y2 = norm2(x1; part_in = p1)    f = FFN(y2)        out = f gamma + x1   (training: part_out, where asked for)
//   backward  df, dgamma = scale_res_bwd(f, dout)      dy2 = FFN'(y2, df)       dx1 = norm2'(x1, dy2) + dout
//             dm, dbeta  = scale_res_bwd(m, dx1)       dy1 = Mixer'(y1, dm)     dx  = norm1'(x, dy1) + dx1
// The seam saves the second BatchNorm its statistics pass (and, in a Stage, the first one's: block i's part_out is block i + 1's
// part_in); the two residual gradients ride in the BatchNorm backwards' last pass (dres).  Eval mode produces and consumes no pairs.
// Bitwise: the results are those of the six calls made one by one, because they ARE those calls.
#include "internal.h"

namespace mi {
namespace {

constexpr int SB_MAX_DIM = 128, SB_MIN_HW = 2, SB_MAX_HW = 512;
// the sub-modules' workspaces share one region (the calls are sequential on one stream); the pairs of x1; the backward's three
// planes; the intermediates of a forward that is given no blob
enum { BW_SUB = 0, BW_P1, BW_D0, BW_D1, BW_D2, BW_SCRATCH, BW_SECTIONS };
enum { BV_Y1 = 0, BV_M, BV_X1, BV_Y2, BV_F, BV_STAT1, BV_STAT2, BV_MIXER, BV_FFN, BV_SECTIONS };
struct SbPlan {
  int B, dim, H, W, dtype, training;
  int64_t N;
  int nchunk;                                    // chunks per plane of the BatchNorm kernels
  int64_t kernels_fwd, kernels_fwd_part_in, kernels_bwd;   // own launches of the six calls, summed from their plans
  int64_t sub_lib_fwd, sub_lib_bwd;              // library calls the Mixer and the FFN make in turn
  size_t pair_bytes, ws_bn, ws_sr, ws_mixer, ws_ffn;
  mi_bn2d_shape bn;
  mi_sfh_mixer_shape mix;
  mi_sfh_ffn_shape ffn;
  Sections<BW_SECTIONS> ws;
  Sections<BV_SECTIONS> saved;
};

int sb_check(const char* who, const mi_sfh_block_shape* s, SbPlan* p) {
  MI_CHECK_ARG(s, "%s: null shape", who);
  const int B = s->B, dim = s->dim, H = s->H, W = s->W, dt = s->dtype;
  MI_CHECK_ARG(dt == MI_F32 || dt == MI_BF16, "%s: bad dtype %d", who, dt);
  MI_CHECK_ARG(B >= 1 && B <= 65535, "%s: bad shape B=%d (1..65535)", who, B);
  MI_CHECK_ARG(dim >= 2 && dim <= SB_MAX_DIM, "%s: dim=%d outside the supported 2..%d", who, dim, SB_MAX_DIM);
  MI_CHECK_ARG(dim % 2 == 0, "%s: dim=%d is odd: not covered (the reference's chunk count changes)", who, dim);
  MI_CHECK_ARG(H >= SB_MIN_HW && H <= SB_MAX_HW, "%s: H=%d outside the supported %d..%d", who, H, SB_MIN_HW, SB_MAX_HW);
  MI_CHECK_ARG(W >= SB_MIN_HW && W <= SB_MAX_HW, "%s: W=%d outside the supported %d..%d", who, W, SB_MIN_HW, SB_MAX_HW);
  memset(p, 0, sizeof(*p));
  p->B = B; p->dim = dim; p->H = H; p->W = W; p->dtype = dt; p->training = s->training ? 1 : 0;
  p->N = (int64_t)H * W;
  p->bn = mi_bn2d_shape{B, dim, H, W, dt, p->training, s->eps, s->momentum};
  p->mix = mi_sfh_mixer_shape{B, dim, H, W, dt, p->training, s->eps, s->momentum};
  p->ffn = mi_sfh_ffn_shape{B, dim, H, W, dt};
  // the parts' own plans: their refusals (eps, momentum, the count, the sizes) stand with their own messages
  int64_t bn[64], sr[64], mx[64], ff[64];
  MI_TRY(mi_bn2d_plan(&p->bn, bn));
  MI_TRY(mi_scale_res_plan(&p->bn, sr));
  MI_TRY(mi_sfh_mixer_plan(&p->mix, mx));
  MI_TRY(mi_sfh_ffn_plan(&p->ffn, ff));
  p->nchunk = (int)bn[7];
  p->pair_bytes = (size_t)bn[62];
  p->ws_bn = (size_t)bn[60]; p->ws_sr = (size_t)sr[60]; p->ws_mixer = (size_t)mx[60]; p->ws_ffn = (size_t)ff[60];
  const int64_t mid = mx[10] + ff[16] + 2 * sr[13];          // the Mixer's, the FFN's and the two residuals' forward launches
  p->kernels_fwd = bn[13] + (p->training ? bn[14] : bn[13]) + mid;   // norm2 always has the pairs of x1 in training mode
  p->kernels_fwd_part_in = 2 * bn[14] + mid;
  p->kernels_bwd = 2 * bn[15] + 2 * sr[15] + mx[11] + ff[17];
  p->sub_lib_fwd = mx[12] + ff[18];
  p->sub_lib_bwd = mx[13] + ff[19];

  const size_t plane = (size_t)B * dim * (size_t)p->N * dtype_size(dt), stat = (size_t)bn[61];
  Sections<BV_SECTIONS>& sv = p->saved;
  for (int i = BV_Y1; i <= BV_F; ++i) sv.put(i, plane);
  sv.put(BV_STAT1, stat); sv.put(BV_STAT2, stat);
  sv.put(BV_MIXER, (size_t)mx[61]); sv.put(BV_FFN, (size_t)ff[61]);
  Sections<BW_SECTIONS>& ws = p->ws;
  ws.put(BW_SUB, max_of({p->ws_bn, p->ws_sr, p->ws_mixer, p->ws_ffn}));
  ws.put(BW_P1, p->training ? p->pair_bytes : 0);
  ws.put(BW_D0, plane); ws.put(BW_D1, plane); ws.put(BW_D2, plane);
  ws.put(BW_SCRATCH, sv.off[BV_MIXER]);                      // y1, m, x1, y2, f and the two stats: the blob without the parts' blobs
  return MI_OK;
}

bool mixer_ok(const mi_sfh_mixer_params& q) {
  return q.cd1_w && q.cd1_b && q.cd2_w && q.cd2_b && q.init_w && q.init_b && q.fina_w && q.fina_b && q.bn_w && q.bn_b && q.fdc_w &&
         q.fdc_b && q.gate_w && q.gate_b && q.fpe_w && q.fpe_b && q.cac_w && q.cac_b && q.ca1_w && q.ca1_b && q.ca2_w && q.ca2_b &&
         q.conv_w && q.conv_b;
}
bool ffn_ok(const mi_sfh_ffn_params& q) {
  return q.init_w && q.init_b && q.c1_w && q.c1_b && q.c2_w && q.c2_b && q.c3_w && q.c3_b && q.fina_w && q.fina_b;
}
bool params_ok(const mi_sfh_block_params* q) {
  return q && q->bn1_w && q->bn1_b && mixer_ok(q->mixer) && q->beta && q->bn2_w && q->bn2_b && ffn_ok(q->ffn) && q->gamma;
}
bool grads_ok(const mi_sfh_block_grads* g) {
  if (!g) return false;
  const mi_sfh_mixer_grads& m = g->mixer;
  const mi_sfh_ffn_grads& f = g->ffn;
  return g->bn1_w && g->bn1_b && g->beta && g->bn2_w && g->bn2_b && g->gamma && m.cd1_w && m.cd1_b && m.cd2_w && m.cd2_b && m.init_w &&
         m.init_b && m.fina_w && m.fina_b && m.bn_w && m.bn_b && m.fdc_w && m.fdc_b && m.gate_w && m.gate_b && m.fpe_w && m.fpe_b &&
         m.cac_w && m.cac_b && m.ca1_w && m.ca1_b && m.ca2_w && m.ca2_b && m.conv_w && m.conv_b && f.init_w && f.init_b && f.c1_w &&
         f.c1_b && f.c2_w && f.c2_b && f.c3_w && f.c3_b && f.fina_w && f.fina_b;
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" size_t mi_sfh_block_workspace(const mi_sfh_block_shape* s) {
  SbPlan p;
  return sb_check("sfh_block_workspace", s, &p) == MI_OK ? p.ws.total : 0;
}
extern "C" size_t mi_sfh_block_saved_bytes(const mi_sfh_block_shape* s) {
  SbPlan p;
  return sb_check("sfh_block_saved_bytes", s, &p) == MI_OK ? p.saved.total : 0;
}
// 12 scalars, the BW_* sections from [16], the BV_* sections of the saved blob from [32] (the format: plan_report, internal.h)
extern "C" int mi_sfh_block_plan(const mi_sfh_block_shape* s, int64_t* out) {
  MI_CHECK_ARG(out, "sfh_block_plan: null pointer");
  SbPlan p;
  MI_TRY(sb_check("sfh_block_plan", s, &p));
  return plan_report<16, 32>(out, {p.B, p.dim, p.N, p.nchunk, 6, 6, 6, p.kernels_fwd, p.kernels_fwd_part_in, p.kernels_bwd, p.sub_lib_fwd,
                                   p.sub_lib_bwd},
                             p.ws, p.saved, {(int64_t)p.ws.total, (int64_t)p.saved.total, (int64_t)p.pair_bytes});
}

extern "C" int mi_sfh_block_fwd(const mi_sfh_block_shape* s, const mi_sfh_block_params* pr, const void* x, void* out,
                                const mi_sfh_block_stats* stats, const float* part_in, float* part_out, void* saved, void* ws,
                                void* stream) {
  SbPlan p;
  MI_TRY(sb_check("sfh_block_fwd", s, &p));
  MI_CHECK_ARG(params_ok(pr) && x && out && ws, "sfh_block_fwd: null pointer");
  MI_CHECK_ARG(stats && stats->mean1 && stats->var1 && stats->mean2 && stats->var2 && stats->mean_fu && stats->var_fu,
               "sfh_block_fwd: null running statistic");
  void* base = saved ? saved : p.ws.at<void>(ws, BW_SCRATCH);
  const Sections<BV_SECTIONS>& sv = p.saved;
  void* y1 = sv.at<void>(base, BV_Y1);
  void* m = sv.at<void>(base, BV_M);
  void* x1 = sv.at<void>(base, BV_X1);
  void* y2 = sv.at<void>(base, BV_Y2);
  void* f = sv.at<void>(base, BV_F);
  void* sub = p.ws.at<void>(ws, BW_SUB);
  float* p1 = p.training ? p.ws.at(ws, BW_P1) : nullptr;
  if (!p.training) { part_in = nullptr; part_out = nullptr; }
  MI_TRY(mi_bn2d_fwd(&p.bn, pr->bn1_w, pr->bn1_b, x, y1, stats->mean1, stats->var1, sv.at(base, BV_STAT1), part_in, sub, stream));  // :273
  MI_TRY(mi_sfh_mixer_fwd(&p.mix, &pr->mixer, y1, m, stats->mean_fu, stats->var_fu, saved ? sv.at<void>(saved, BV_MIXER) : nullptr,
                          sub, stream));                                                                                        // :274
  MI_TRY(mi_scale_res_fwd(&p.bn, pr->beta, m, x, x1, p1, stream));                                                              // :275
  MI_TRY(mi_bn2d_fwd(&p.bn, pr->bn2_w, pr->bn2_b, x1, y2, stats->mean2, stats->var2, sv.at(base, BV_STAT2), p1, sub, stream));   // :278
  MI_TRY(mi_sfh_ffn_fwd(&p.ffn, &pr->ffn, y2, f, saved ? sv.at<void>(saved, BV_FFN) : nullptr, sub, stream));                    // :279
  return mi_scale_res_fwd(&p.bn, pr->gamma, f, x1, out, part_out, stream);                                                      // :280
}

extern "C" int mi_sfh_block_bwd(const mi_sfh_block_shape* s, const mi_sfh_block_params* pr, const void* x, const void* dout, void* dx,
                                const mi_sfh_block_grads* gr, const void* saved, void* ws, void* stream) {
  SbPlan p;
  MI_TRY(sb_check("sfh_block_bwd", s, &p));
  MI_CHECK_ARG(params_ok(pr) && x && dout && dx && saved && ws, "sfh_block_bwd: null pointer");
  MI_CHECK_ARG(grads_ok(gr), "sfh_block_bwd: null gradient buffer");
  const Sections<BV_SECTIONS>& sv = p.saved;
  const int acc = gr->accumulate ? 1 : 0;
  mi_sfh_mixer_grads mg = gr->mixer;
  mi_sfh_ffn_grads fg = gr->ffn;
  mg.accumulate = acc; fg.accumulate = acc;
  void* sub = p.ws.at<void>(ws, BW_SUB);
  void* d0 = p.ws.at<void>(ws, BW_D0);
  void* d1 = p.ws.at<void>(ws, BW_D1);
  void* d2 = p.ws.at<void>(ws, BW_D2);
  MI_TRY(mi_scale_res_bwd(&p.bn, pr->gamma, sv.at<void>(saved, BV_F), dout, d0, gr->gamma, acc, sub, stream));                   // df
  MI_TRY(mi_sfh_ffn_bwd(&p.ffn, &pr->ffn, sv.at<void>(saved, BV_Y2), d0, d1, &fg, sv.at<void>(saved, BV_FFN), sub, stream));     // dy2
  MI_TRY(mi_bn2d_bwd(&p.bn, pr->bn2_w, sv.at<void>(saved, BV_X1), d1, dout, d2, gr->bn2_w, gr->bn2_b, acc, sv.at(saved, BV_STAT2), sub,
                     stream));                                                                                                  // dx1
  MI_TRY(mi_scale_res_bwd(&p.bn, pr->beta, sv.at<void>(saved, BV_M), d2, d0, gr->beta, acc, sub, stream));                       // dm
  MI_TRY(mi_sfh_mixer_bwd(&p.mix, &pr->mixer, sv.at<void>(saved, BV_Y1), d0, d1, &mg, sv.at<void>(saved, BV_MIXER), sub, stream));   // dy1
  return mi_bn2d_bwd(&p.bn, pr->bn1_w, x, d1, d2, dx, gr->bn1_w, gr->bn1_b, acc, sv.at(saved, BV_STAT1), sub, stream);
}
