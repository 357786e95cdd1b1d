/*
 * mi_restore.h — C-ABI of the MI355X (gfx950) Restormer / MoCE-IR block library.
 *
 * Drop-in boundary for the hot path named in BASELINE.json: the reference has no
 * FFI of its own (it is pure PyTorch), so every entry point below replaces the
 * ATen/cuDNN/cuBLAS kernels that one reference nn.Module.forward()/autograd
 * backward launches.  The reference interface each entry point stands behind is
 * cited as file:line relative to the upstream repository root.
 *
 * Conventions:
 *  - plain pointers and sizes only; no torch types.  All pointers are DEVICE
 *    pointers unless said otherwise.  The caller owns every buffer (inputs,
 *    outputs, saved-for-backward blobs, workspaces); the library never
 *    allocates or frees device memory and keeps no pointer past return.
 *  - activations are NCHW contiguous, dtype MI_F32 or MI_BF16; parameters and
 *    parameter gradients are always fp32 in the reference's (PyTorch conv)
 *    layout: 1x1 conv [Cout,Cin], depthwise [C,k*k], LayerNorm [C].
 *  - every call takes the HIP stream to launch on (hipStream_t as void*).
 *  - return 0 on success, negative on failure; mi_last_error() gives the
 *    message (thread local).  No exceptions or aborts cross the ABI.
 *  - thread-safe: no global mutable state except the thread-local error string,
 *    the profiler and the opt-in packed-weight cache (mi_pw_cache_*), both mutex
 *    protected (backward is called from autograd worker threads).
 */
#ifndef MI_RESTORE_H
#define MI_RESTORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_RESTORE_VERSION 100

typedef enum { MI_F32 = 0, MI_BF16 = 1 } mi_dtype;

enum {
  MI_OK = 0,
  MI_ERR_ARG = -1,      /* bad shape / dtype / null pointer / unsupported size */
  MI_ERR_ALIGN = -2,    /* pointer not aligned as required */
  MI_ERR_HIP = -3       /* a HIP runtime call failed */
};

int mi_version(void);
const char* mi_last_error(void);
/* The MI_* A/B switches (environment variables consulted by the launch planners) are read once, at first use.  This re-reads
 * them: for tests and A/B tools that flip a switch inside one process.  Not meant to race with launches on other threads. */
int mi_env_reload(void);

/* Deferred parameter-gradient reductions.  Every weight gradient of the blocks ends in a fixed-order sum of partial rows into
 * the gradient buffer; as separate launches that was ~500 kernels of 5-15 us per training step.  Between mi_deferred_begin and
 * mi_deferred_end, backward entry points called with accumulate != 0 place those partials in the lent arena (device memory,
 * caller-owned, >= 2 MiB; a few GiB for a Restormer-base step - when it is full the entry points fall back to immediate sums)
 * and record the sum instead of launching it; mi_deferred_flush(stream) runs everything recorded so far in one table-driven
 * launch on `stream` (the stream the backward ran on), in a fixed order per gradient (bitwise reproducible), and
 * recycles the arena.  Contract: nothing reads such a gradient buffer between the backward call and the flush (the trainer
 * switches recording on in zero_grad() and flushes + switches it off before its all-reduce / optimizer step).  One context per
 * process. */
int mi_deferred_begin(void* arena, size_t bytes);
int mi_deferred_record(int on);         /* producers defer only while recording is on (the owner's backward window); begin() leaves it off */
int mi_deferred_pending(void);          /* reductions recorded and not yet flushed */
size_t mi_deferred_high_water(void);    /* most arena bytes in use at once since the library was loaded (sizing aid) */
int mi_deferred_flush(void* stream);
int mi_deferred_end(void);

/* ------------------------------------------------------------------------
 * Channel LayerNorm on NCHW  (Restormer.py:25-70; moce_ir.py:156-221;
 * AdaIR-main/net/model.py:25-71).  with_bias=1: (x-mu)/sqrt(var+1e-5)*w+b ;
 * with_bias=0 ("BiasFree"): x/sqrt(var+1e-5)*w, var about the mean.
 * mean/rstd: [B, H*W] fp32, written by fwd (may be NULL), read by bwd.
 * bwd: dx = LN'(dy) (+ dres if non-NULL);  dw/db are accumulated (+=) when
 * accumulate!=0, else overwritten.  ws: mi_ln_bwd_workspace() bytes.
 * ------------------------------------------------------------------------ */
int mi_ln_fwd(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd,
              int B, int C, int64_t N, int with_bias, int dtype, void* stream);
/* The same with the caller's eps, 0 < eps < 1 (DarkIR's LayerNorm2d: 1e-6, arch_util.py:37).  mi_ln_fwd is this call with 1e-5:
 * one set of kernels, eps a kernel argument.  The backward reads the saved rstd and needs no eps. */
int mi_ln_fwd_eps(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd,
                  int B, int C, int64_t N, int with_bias, float eps, int dtype, void* stream);
size_t mi_ln_bwd_workspace(int B, int C, int64_t N);
int mi_ln_bwd(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
              const void* dres, void* dx, float* dw, float* db,
              int B, int C, int64_t N, int with_bias, int accumulate, int dtype,
              void* ws, void* stream);
/* What mi_ln_fwd (backward = 0) / mi_ln_bwd (1) launch for this call (read-only; honours MI_LN_FORM).  aligned: every activation
 * pointer of the call is a multiple of 4 bytes (bf16 then moves two pixels per lane when N is even).
 * out[9] = {family (0 block, 1 wave-owned), waves per workgroup | channels per slice CB, channels per thread CPT | waves per
 *           tile WS, 0 | waves per workgroup NW, pixels per lane, pixel tiles per workgroup, grid x, partial rows (backward),
 *           1 when the row reduction takes two stages (backward, outside a deferred window)}. */
int mi_ln_plan(int B, int C, int64_t N, int dtype, int backward, int aligned, int* out);

/* ------------------------------------------------------------------------
 * Depthwise k x k convolution, stride 1, zero pad k/2, groups = channels
 * (Restormer.py:84,106 3x3; moce_ir.py:341 7x7).  w: [C, k*k], bias [C] or NULL.
 *  fwd      : y = dw(x)
 *  fwd_gate : C = 2h channels; y (may be NULL) = dw(x) [B,2h,H,W];
 *             g = gelu_erf(y[:, :h]) * y[:, h:]  [B,h,H,W]   (Restormer.py:90-91)
 *  bwd      : dx = dw^T(dy);  dw/db accumulated or overwritten.
 *  bwd_gate : same, with dy of the 2h conv outputs formed on the fly from
 *             (dg [B,h,H,W], y [B,2h,H,W]) — the GELU-gate backward.
 * ------------------------------------------------------------------------ */
int mi_dwconv_fwd(const void* x, const float* w, const float* bias, void* y,
                  int B, int C, int H, int W, int ks, int dtype, void* stream);
int mi_dwconv_gate_fwd(const void* x, const float* w, const float* bias, void* y, void* g,
                       int B, int C2, int H, int W, int ks, int dtype, void* stream);
size_t mi_dwconv_bwd_workspace(int B, int C, int H, int W, int ks);
int mi_dwconv_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db,
                  int B, int C, int H, int W, int ks, int accumulate, int dtype, void* ws, void* stream);
int mi_dwconv_gate_bwd(const void* dg, const void* y, const void* x, const float* w, void* dx, float* dw,
                       float* db, int B, int C2, int H, int W, int ks, int accumulate, int dtype,
                       void* ws, void* stream);
/* GDFN gate backward WITHOUT stored conv outputs: y1, y2 are recomputed from the conv input x inside the kernel (the
 * input rows are needed for the weight gradient anyway), so the forward need not write y at all (mi_dwconv_gate_fwd with
 * y = NULL) - a third less HBM traffic over the depthwise stage and 2h fewer saved planes.  Available for the shapes
 * mi_dwconv_gate_recompute_ok() reports (3x3, rows of 16..256 pixels, power of two); same workspace as mi_dwconv_gate_bwd. */
int mi_dwconv_gate_recompute_ok(int H, int W, int ks);
/* The launch plan the depthwise entry points take for 16-byte-aligned planes (read-only; honours MI_DW_LDS).
 * op: 0 fwd, 1 gate fwd, 2 bwd (every form), 3 gate bwd (stored or recomputed y); the gate ops work on B*C/2 planes.
 * out[6] = {family (0 LDS-tiled, 1 register-streaming), band rows | tile rows, bands per plane, lanes per row | tile width,
 *           uni (streaming: one plane per wave), rows per lane | rows per thread}. */
int mi_dwconv_plan(int B, int C, int H, int W, int ks, int op, int* out);
int mi_dwconv_gate_bwd_recompute(const void* dg, const void* x, const float* w, const float* bias, void* dx, float* dw,
                                 float* db, int B, int C2, int H, int W, int ks, int accumulate, int dtype, void* ws,
                                 void* stream);

/* ------------------------------------------------------------------------
 * Pointwise (1x1 conv) GEMM on N-contiguous planes (Restormer.py:82,86,105,107):
 *   Y[z][m][n] = sum_k Wz(m,k) * X[z][k][n]  (+ bias[m]) (+ R[z][m][n])
 * z = batch*groups + group.  X may be given as two K-panels (X1 rows 0..K1-1,
 * X2 rows K1..K1+K2-1): concat-free 1x1 over a channel concat.
 * Weight element (m,k) of slice z lives at W[b*w_bs + g*w_gs + m*w_sm + k*w_sk]
 * (w_sk==1: row-major [M,K]; w_sm==1: the transpose of a [K,M] matrix).
 * Strides are in elements.  ws: mi_pw_gemm_workspace() bytes (16-byte aligned); it receives the
 * weights re-packed into the kernel's LDS image (activation dtype), written and read by this call only.
 * ------------------------------------------------------------------------ */
typedef struct {
  const void* x1; int64_t x1_bs, x1_gs; int k1;
  const void* x2; int64_t x2_bs, x2_gs; int k2;   /* x2 may be NULL (k2 = 0) */
  const float* w; int64_t w_bs, w_gs, w_sm, w_sk;
  const float* bias; int64_t bias_gs;             /* may be NULL */
  const void* r; int64_t r_bs, r_gs;              /* residual, may be NULL */
  void* y; int64_t y_bs, y_gs;
  int m; int64_t n; int batch; int groups; int dtype;
  /* Optional LayerNorm over the K channels of X1, applied as the tile is loaded (Restormer.py:27-70 in front of :89 / :115):
   * ln_mode 0 = none, 1 = WithBias ((x - mu) rstd w + b), 2 = BiasFree (x rstd w); ln_w / ln_b [K]; ln_mean / ln_rstd
   * [batch, n] receive the statistics (both or neither).  Only where mi_pw_gemm_ln_ok() says so (the X-resident kernels:
   * bf16; 96 < M with K <= 96, or 256 <= M with K <= 128; one K panel, one group); zero-initialise the struct to leave it off. */
  const float* ln_w; const float* ln_b; float* ln_mean; float* ln_rstd; int ln_mode;
  /* Optional fp8 (OCP e4m3) MFMA operands - the "CDNA4 fp8 MFMA projections" of the tiled-inference configuration (BASELINE
   * configs[4]); inference only.  f8 = 1: X (after the optional LayerNorm) is divided by f8_sx and W (its packed bf16 image)
   * by f8_sw, both are rounded to e4m3 in registers (saturating at +-448) and multiplied with v_mfma_f32_16x16x32_fp8_fp8; the fp32 accumulator
   * is scaled back by f8_sx * f8_sw before bias / residual.  The hardware conversion uses the scales' exponents only: pass
   * powers of two, chosen so that |X| / f8_sx and |W| / f8_sw stay <= 448.  X, Y and the residual stay bf16 in HBM.  Only
   * where mi_pw_gemm_f8_ok() says so (the wave-owned bf16 kernels); zero-initialise the struct to leave it off. */
  int f8; float f8_sx, f8_sw;
  /* Optional second output: rows m >= y_split of the result are written to y2 (row m - y_split), the rows below to y - two
   * results of ONE pass over X (the q and k gradients of MDTA, which multiply the same q, k planes with two per-image
   * matrices).  No residual; only where mi_pw_gemm_split_ok() says so (the wave-owned bf16 kernels); zero = off. */
  int y_split; void* y2; int64_t y2_bs, y2_gs;
  /* Optional bf16 copy of PER-IMAGE weights (w_bs != 0): the same matrix values as `w`, already rounded to bf16, row-major
   * [m][k] with unit k stride and row stride w_b16_sm (elements), batch / group strides w_bs / w_gs as for `w` (all multiples of
   * 8, 16-byte aligned).  The wave-owned bf16 kernels then stage the weights straight from it and no pack launch runs (the
   * producers of such matrices - the c x c attention fold, the q / k gradient matrices - write both).  `w` must stay valid: the
   * other kernel forms pack from it.  NULL = off. */
  const void* w_b16; int64_t w_b16_sm;
} mi_pw_desc;
size_t mi_pw_gemm_workspace(const mi_pw_desc* d);
int mi_pw_gemm(const mi_pw_desc* d, void* ws, void* stream);
int mi_pw_gemm_ln_ok(const mi_pw_desc* d);
int mi_pw_gemm_f8_ok(const mi_pw_desc* d);
int mi_pw_gemm_split_ok(const mi_pw_desc* d);
/* What mi_pw_gemm runs for d under the current A/B switches (host-only; the pointers are read for their 16-byte alignment only,
 * so placeholders will do).  out[18]: family (0 chunked, 1 weight-resident, 2 LDS-DMA, 3 wave X-resident, 4 wave stream, 5 wave
 * X-wide, 6 LDS-tiled deep K), tile rows, K chunks, fp8, LayerNorm on load, grid x, y, z, block, dynamic LDS bytes, pixel tiles
 * per wave, pixel tiles per workgroup, X-wide slabs, slabs per workgroup, XCD map, weight source (0 own pack, 1 bf16 copy,
 * 2 direct fp32), may use the pack cache, workspace bytes. */
int mi_pw_plan(const mi_pw_desc* d, int64_t* out);

/* Opt-in packed-weight cache.  By default every mi_pw_gemm (and every module entry point built on it) packs its weight
 * matrix into its own workspace, once per call, and the library keeps no state.  A caller that controls when the
 * weights change (a trainer: only at the optimizer step; an inference server: never) may lend a device buffer:
 *   mi_pw_cache_enable(buf, bytes, lo, hi)  buf stays owned by the caller and must outlive the cache; NULL disables it.
 *                                   Only weights whose address lies in [lo, hi) - the caller's parameter storage - are
 *                                   cached: a temporary weight matrix (a permuted copy, ...) may reuse an address with
 *                                   different values and always packs per call.
 *   mi_pw_cache_refresh(stream)     re-packs EVERY weight seen so far in one launch; from then on calls with those
 *                                   weights skip their pack launch.  Call it after each optimizer step (the weights
 *                                   registered since the last refresh are picked up; the first refresh after new
 *                                   registrations must run outside stream capture).
 *   mi_pw_cache_invalidate()        packed images are stale (weights were overwritten some other way): calls pack
 *                                   per call again until the next refresh.
 * Per-image weights (w_bs != 0) are never cached.  The cache is process-global and mutex-protected; this is the only
 * mutable state in the library besides the thread-local error string and the profiler.                              */
int mi_pw_cache_enable(void* buf, size_t bytes, const void* params_lo, const void* params_hi);
int mi_pw_cache_refresh(void* stream);
int mi_pw_cache_invalidate(void);
int mi_pw_cache_pending(void);   /* 1 while weights registered since the last refresh (or an invalidation) wait for one */

/* ------------------------------------------------------------------------
 * Row-Gram (reduction over the pixel axis), the contraction of MDTA's q k^T
 * (Restormer.py:124) and of every 1x1-conv weight gradient:
 *   G[z][i][j] = sum_n A[z][i][n] * Bm[z][j][n]
 * optionally summed over the batch index, optionally also the row sums of
 * squares of A and Bm (for F.normalize, Restormer.py:121-122).
 * Split over n across workgroups with a deterministic two-stage reduce.
 * out = (accumulate? out : 0) + G.   ws: mi_gram_workspace() bytes.
 * ------------------------------------------------------------------------ */
typedef struct {
  const void* a; int64_t a_bs, a_gs; int ma;
  const void* b; int64_t b_bs, b_gs; int mb;
  int64_t n; int batch; int groups; int dtype;
  int sum_batch;           /* 1: out is [groups, ma, mb] summed over batch */
  int accumulate;          /* 1: out += */
  float* out;              /* [batch*groups or groups][ma][mb]; row stride out_ld (>= mb) */
  int64_t out_ld, out_zs;  /* row stride / slice stride of out, elements */
  float* sumsq;            /* NULL or [batch*groups][ma+mb] */
} mi_gram_desc;
size_t mi_gram_workspace(const mi_gram_desc* d);
int mi_gram(const mi_gram_desc* d, void* ws, void* stream);
/* What mi_gram runs for d under the current A/B switches (host-only; the pointers are read for their 16-byte alignment only, so
 * placeholders will do).  out[22]: family (0 LDS-staged, 1 streaming), fragments per tile side over A and over B (32 rows each;
 * streaming: 16), sumsq, contraction unit in pixels, units in total, units per split, splits, tiles over A, tiles over B, Z
 * (slices of partials), fold (units per image when the batch is chained along the pixel axis, else 0), 16-byte rows, grid x, y, z,
 * block, partial bytes, sumsq row bytes, finish (0 direct into the output, 1 reduce few<4>, 2 reduce few<16>, 3 general reduce),
 * partials may go to the deferred arena, workspace bytes of this plan (sumsq rows reserved). */
int mi_gram_plan(const mi_gram_desc* d, int64_t* out);

/* ------------------------------------------------------------------------
 * MDTA — Attention.forward / backward  (Restormer.py:99-132; moce_ir.py:283-321;
 * AdaIR-main/net/model.py:99-130).  out = (residual?) + project_out(attn(qkv_dw(qkv(x)))).
 * saved: mi_mdta_saved_bytes() blob written by fwd when non-NULL (training),
 * read by bwd.  ws: mi_mdta_workspace() bytes scratch.
 * Gradients are accumulated (+=) when accumulate!=0, else overwritten; NULL
 * bias pointers mean the conv has no bias.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, heads, H, W, dtype, ks; } mi_mdta_shape;
typedef struct {
  const float* temperature;                 /* [heads] */
  const float* qkv_w;  const float* qkv_b;  /* [3C,C], [3C]|NULL */
  const float* dw_w;   const float* dw_b;   /* [3C,ks*ks], [3C]|NULL */
  const float* proj_w; const float* proj_b; /* [C,C], [C]|NULL */
} mi_mdta_params;
typedef struct {
  float* temperature; float* qkv_w; float* qkv_b; float* dw_w; float* dw_b; float* proj_w; float* proj_b;
  int accumulate;
} mi_mdta_grads;
size_t mi_mdta_saved_bytes(const mi_mdta_shape* s);
size_t mi_mdta_workspace(const mi_mdta_shape* s);
int mi_mdta_fwd(const mi_mdta_shape* s, const mi_mdta_params* p, const void* x, const void* residual,
                void* out, void* saved, void* ws, void* stream);
int mi_mdta_bwd(const mi_mdta_shape* s, const mi_mdta_params* p, const void* x, const void* dout,
                void* dx, const mi_mdta_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * Cross-MDTA: q from x (1x1 C->C + depthwise ks_q), k,v from y (1x1 C->2C + depthwise ks_kv), then the
 * MDTA core.  moce_ir.py:325-368 CrossAttention (ks_q 3, ks_kv 7); AdaIR-main/net/model.py:177-216
 * Chanel_Cross_Attention (3, 3).  bwd returns dx and dy.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, heads, H, W, dtype, ks_q, ks_kv; } mi_xmdta_shape;
typedef struct {
  const float* temperature;
  const float* q_w;  const float* q_b;  const float* q_dw_w;  const float* q_dw_b;     /* [C,C] [C] [C,ks_q^2] [C] */
  const float* kv_w; const float* kv_b; const float* kv_dw_w; const float* kv_dw_b;    /* [2C,C] [2C] [2C,ks_kv^2] [2C] */
  const float* proj_w; const float* proj_b;
} mi_xmdta_params;
typedef struct {
  float* temperature; float* q_w; float* q_b; float* q_dw_w; float* q_dw_b; float* kv_w; float* kv_b; float* kv_dw_w;
  float* kv_dw_b; float* proj_w; float* proj_b; int accumulate;
} mi_xmdta_grads;
size_t mi_xmdta_saved_bytes(const mi_xmdta_shape* s);
size_t mi_xmdta_workspace(const mi_xmdta_shape* s);
int mi_xmdta_fwd(const mi_xmdta_shape* s, const mi_xmdta_params* p, const void* x, const void* y,
                 const void* residual, void* out, void* saved, void* ws, void* stream);
int mi_xmdta_bwd(const mi_xmdta_shape* s, const mi_xmdta_params* p, const void* x, const void* y, const void* dout,
                 void* dx, void* dy, const mi_xmdta_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * TKSA — DRSformer's top-k sparse attention, Attention.forward / backward (DRSformer_arch.py:101-171).  MDTA's qkv 1x1, 3x3
 * depthwise, L2-normalised q, k, temperature and project_out; the c x c map is A = sum_m attn_m softmax(top-k_m(S)) with
 * S = temperature * cos(q, k): in each row of S only the k_m largest entries stay, the rest are -inf (ties: lower column index
 * first).  c = C/heads <= 120; k1..k4 in 1..c (DRSformer: int(c/2), int(c*2/3), int(c*3/4), int(c*4/5), computed by the
 * caller).  mi_mdta_params / mi_mdta_grads carry the MDTA parameters (the depthwise conv is 3x3); mi_tksa_params /
 * mi_tksa_grads the four [1] mixing weights.  scores: NULL or [B, heads, c, c] fp32, receives the S the masks were ranked
 * from.  The attn_m gradients follow mi_mdta_grads.accumulate.  Sizing entry points return 0 for a shape not covered.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, heads, H, W, dtype, k1, k2, k3, k4; } mi_tksa_shape;
typedef struct { const float* attn1; const float* attn2; const float* attn3; const float* attn4; } mi_tksa_params;
typedef struct { float* attn1; float* attn2; float* attn3; float* attn4; } mi_tksa_grads;
size_t mi_tksa_saved_bytes(const mi_tksa_shape* s);
size_t mi_tksa_workspace(const mi_tksa_shape* s);
int mi_tksa_fwd(const mi_tksa_shape* s, const mi_mdta_params* p, const mi_tksa_params* tp, const void* x, const void* residual,
                void* out, void* saved, void* ws, float* scores, void* stream);
int mi_tksa_bwd(const mi_tksa_shape* s, const mi_mdta_params* p, const mi_tksa_params* tp, const void* x, const void* dout,
                void* dx, const mi_mdta_grads* g, const mi_tksa_grads* tg, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * MSFN — DRSformer's mixed-scale FeedForward.forward / backward (DRSformer_arch.py:62-98).  hidden = h:
 *   h0 = project_in(x) [2h];  a = relu(dwconv3x3(h0)), b = relu(dwconv5x5(h0)) (depthwise, 2h each);
 *   y1 = relu(dwconv3x3_1(cat(a[:h], b[:h]))), y2 = relu(dwconv5x5_1(cat(a[h:], b[h:]))) (groups = h, two inputs per group);
 *   out = (residual?) + project_out(cat(y1, y2)).
 * Any h (odd h: one group reads the last channel of a and the first of b).  NULL biases: the convs have none.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, hidden, H, W, dtype; } mi_msfn_shape;
typedef struct {
  const float* in_w;  const float* in_b;   /* [2h,C], [2h]|NULL */
  const float* dw3_w; const float* dw3_b;  /* [2h,9], [2h]|NULL */
  const float* dw5_w; const float* dw5_b;  /* [2h,25], [2h]|NULL */
  const float* g3_w;  const float* g3_b;   /* [h,2,9], [h]|NULL */
  const float* g5_w;  const float* g5_b;   /* [h,2,25], [h]|NULL */
  const float* out_w; const float* out_b;  /* [C,2h], [C]|NULL */
} mi_msfn_params;
typedef struct {
  float* in_w; float* in_b; float* dw3_w; float* dw3_b; float* dw5_w; float* dw5_b; float* g3_w; float* g3_b; float* g5_w;
  float* g5_b; float* out_w; float* out_b; int accumulate;
} mi_msfn_grads;
size_t mi_msfn_saved_bytes(const mi_msfn_shape* s);
size_t mi_msfn_workspace(const mi_msfn_shape* s);
int mi_msfn_fwd(const mi_msfn_shape* s, const mi_msfn_params* p, const void* x, const void* residual,
                void* out, void* saved, void* ws, void* stream);
int mi_msfn_bwd(const mi_msfn_shape* s, const mi_msfn_params* p, const void* x, const void* dout,
                void* dx, const mi_msfn_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * MEFC — one layer pair of DRSformer's Mixture of Experts Feature Compensator (`subnet`, DRSformer_arch.py:328-354): the
 * OALayer routing head (:227-247) and the GroupOLs it weights (:206-225), forward / backward as one unit:
 *   w[b, t, :] = softmax_i(fc2(relu(fc1(mean_hw x[b]))))[t]           (steps x 8 routing weights per image)
 *   s = relu(pre_w . x);  per step t:  s = relu(relu(out_w . cat_i(w[b,t,i] op_i(s))) + s)
 *   ops i = sep1, sep3, sep5, sep7 (SepConv: pw2 . dw2(relu(pw1 . dw1(s)))), dil3, dil5, dil7 (DilConv: pw . dw_dilation2(s)),
 *   avg (3x3 average pool, count_include_pad=False).
 * Any H, W >= 1; 1 <= steps <= 16; C <= 4096.  Parameters and gradients fp32; dw weights [C, k*k], 1x1 weights [C, C] (out_w
 * [C, 8C]); `step` points to a HOST array of `steps` structs.  fwd: out [B, C, H, W]; saved (NULL: inference) receives the
 * planes the backward reads.  bwd takes the forward's output as well (the mask of the last residual ReLU).  NULL is not
 * accepted for any weight (the reference's convs have no bias; its Linears have one).
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, H, W, dtype, steps; } mi_mefc_shape;
typedef struct {
  const float* sep_dw1[4]; const float* sep_pw1[4];  /* SepConv k = 1, 3, 5, 7: op.0 [C, k*k], op.1 [C, C] */
  const float* sep_dw2[4]; const float* sep_pw2[4];  /*                          op.3 [C, k*k], op.4 [C, C] */
  const float* dil_dw[3];  const float* dil_pw[3];   /* DilConv k = 3, 5, 7:     op.0 [C, k*k], op.1 [C, C] */
  const float* out_w;                                /* _out.0 [C, 8C] */
} mi_mefc_step_params;
typedef struct {
  float* sep_dw1[4]; float* sep_pw1[4]; float* sep_dw2[4]; float* sep_pw2[4]; float* dil_dw[3]; float* dil_pw[3]; float* out_w;
} mi_mefc_step_grads;
typedef struct {
  const float* fc1_w; const float* fc1_b;   /* OALayer ca_fc.0: [16 steps, C], [16 steps] */
  const float* fc2_w; const float* fc2_b;   /* ca_fc.2: [8 steps, 16 steps], [8 steps] */
  const float* pre_w;                       /* GroupOLs.preprocess.op.0 [C, C] */
  const mi_mefc_step_params* step;          /* host array [steps] */
} mi_mefc_params;
typedef struct {
  float* fc1_w; float* fc1_b; float* fc2_w; float* fc2_b; float* pre_w;
  const mi_mefc_step_grads* step;           /* host array [steps] */
  int accumulate;
} mi_mefc_grads;
size_t mi_mefc_saved_bytes(const mi_mefc_shape* s);
size_t mi_mefc_workspace(const mi_mefc_shape* s);
int mi_mefc_fwd(const mi_mefc_shape* s, const mi_mefc_params* p, const void* x, void* out, void* saved, void* ws, void* stream);
int mi_mefc_bwd(const mi_mefc_shape* s, const mi_mefc_params* p, const void* x, const void* out, const void* dout, void* dx,
                const mi_mefc_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * DarkIR — the dilated-gate decoder block (DarkIR-main/archs/arch_model.py:72-139 DBlock; Branch :57-70; SimpleGate :12-15).
 *
 * dilgate: the n summed dilated depthwise 3x3 convs of the Branch list on the same 2c planes, SimpleGate and the SCA pool sums:
 *   z = sum_i (dw3x3(x; w_i, dilation d_i, padding d_i) + b_i)   [B,2c,H,W];   g = z[:, :c] * z[:, c:]   [B,c,H,W]
 *   pool[b, j] = sum_hw g[b, j]   (fp32, of the unrounded products; per-tile partials summed in a fixed order: no atomics)
 * 1 <= n_dil <= 4, 1 <= d_i <= 16 (they may repeat), any H, W, c >= 1 (c <= 65535).  w_i [2c, 9], b_i [2c] (NULL: none).
 * One workgroup forms both halves (j, j + c) of a 32-row tile from one LDS tile with a max(d_i) halo.  z is never stored: the
 * backward recomputes it from x.  Its scratch dz is fp32 in either dtype.  fwd ws / bwd ws: mi_dilgate_fwd_workspace / mi_dilgate_bwd_workspace bytes.
 *   bwd: dz[:, :c] = (dg + dg_add[b, j]) z[:, c:], dz[:, c:] = (dg + dg_add[b, j]) z[:, :c]  (dg_add [B, c] fp32 or NULL: the
 *        gradient through the pooled mean, constant over a plane);  dx = sum_i dw_i^T dz;  dw_i, db_i fixed-order sums, added to
 *        the buffers when accumulate != 0, else written (a NULL b[i] is skipped).
 * mi_dilgate_plan (host-only; the launchers take every decision from the same plan) fills out[12]: tile rows, tile columns, halo,
 * dynamic LDS bytes, forward grid x (tiles of a plane), y (c), z (B), pool partials per plane, 1 when z is stored (never), forward
 * workspace bytes, workgroups per (image, channel pair) of the backward's weight-gradient pass, backward workspace bytes.
 *
 * pairconv3x3: DBlock.extra_conv (:83), a 3x3 conv with padding 1 on 2c channels in c groups: output channels 2g, 2g + 1 each read
 * input channels 2g, 2g + 1.  w [2c, 2, 9], bias [2c] or NULL.  bwd: dx, dw, db (db may be NULL).
 * ------------------------------------------------------------------------ */
typedef struct { const float* w[4]; const float* b[4]; } mi_dilgate_params;
typedef struct { float* w[4]; float* b[4]; int accumulate; } mi_dilgate_grads;
int mi_dilgate_plan(int B, int c, int H, int W, int dtype, int n_dil, const int* dil, int64_t* out);
size_t mi_dilgate_fwd_workspace(int B, int c, int H, int W);
int mi_dilgate_fwd(const void* x, const mi_dilgate_params* p, void* g, float* pool, int B, int c, int H, int W, int n_dil,
                   const int* dil, int dtype, void* ws, void* stream);
size_t mi_dilgate_bwd_workspace(int B, int c, int H, int W, int n_dil, int dtype);
int mi_dilgate_bwd(const void* dg, const float* dg_add, const void* x, const mi_dilgate_params* p, void* dx,
                   const mi_dilgate_grads* gr, int B, int c, int H, int W, int n_dil, const int* dil, int dtype, void* ws,
                   void* stream);
int mi_pairconv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int c, int H, int W, int dtype,
                       void* stream);
size_t mi_pairconv3x3_bwd_workspace(int B, int c, int H, int W);
int mi_pairconv3x3_bwd(const void* dy, const void* x, const float* w, void* dx, float* dw, float* db, int B, int c, int H, int W,
                       int accumulate, int dtype, void* ws, void* stream);

/* DBlock.forward / backward as one unit:
 *   x0 = LayerNorm2d(inp; norm1, eps 1e-6);  x1 = conv1(x0) [2c];  x2 = extra_conv(x1) when `extra`, else x1;
 *   g = dilgate(x2);  s[b] = sca_w . mean_hw(g[b]) + sca_b;  y = inp + beta (conv3(s g));
 *   u = conv4(LayerNorm2d(y; norm2));  out = y + gamma conv5(u[:, :c] u[:, c:]).
 * conv3 with the SCA scale, beta and the residual is ONE per-image 1x1 GEMM (M[b] = diag(beta) W3 diag(s[b]), bias beta b3,
 * r = inp); conv5 with gamma and the residual likewise (diag(gamma) W5).  C <= 256 (DarkIR's widest level).
 * With bf16 activations the four 1x1 products and their transposes run on SPLIT weights, [hi | lo] . [x ; x] with hi = w rounded to
 * bf16 and lo = w - hi (two K panels of mi_pw_gemm): the MFMA path would otherwise round each weight to 8 mantissa bits, an error
 * common to a channel that the bias gradients (pixel sums) keep whole.
 * Parameters fp32 in the reference's layout: 1x1 [Cout, Cin], branch [2c, 9], extra_conv [2c, 2, 9], beta / gamma [c]; every bias
 * is required (the reference's convs all have one); extra_w / extra_b are read only when `extra`.  saved == NULL: inference,
 * nothing is kept.  The sizing calls return 0 for a shape that is not covered.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, H, W, dtype, n_dil; int dil[4]; int extra; } mi_dblock_shape;
typedef struct {
  const float* norm1_w; const float* norm1_b; const float* conv1_w; const float* conv1_b; const float* extra_w; const float* extra_b;
  const float* br_w[4]; const float* br_b[4];
  const float* sca_w; const float* sca_b; const float* conv3_w; const float* conv3_b; const float* beta;
  const float* norm2_w; const float* norm2_b; const float* conv4_w; const float* conv4_b; const float* conv5_w; const float* conv5_b;
  const float* gamma;
} mi_dblock_params;
typedef struct {
  float* norm1_w; float* norm1_b; float* conv1_w; float* conv1_b; float* extra_w; float* extra_b;
  float* br_w[4]; float* br_b[4];
  float* sca_w; float* sca_b; float* conv3_w; float* conv3_b; float* beta;
  float* norm2_w; float* norm2_b; float* conv4_w; float* conv4_b; float* conv5_w; float* conv5_b;
  float* gamma;
  int accumulate;
} mi_dblock_grads;
size_t mi_dblock_saved_bytes(const mi_dblock_shape* s);
size_t mi_dblock_workspace(const mi_dblock_shape* s);
int mi_dblock_fwd(const mi_dblock_shape* s, const mi_dblock_params* p, const void* inp, void* out, void* saved, void* ws,
                  void* stream);
int mi_dblock_bwd(const mi_dblock_shape* s, const mi_dblock_params* p, const void* inp, const void* dout, void* dinp,
                  const mi_dblock_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * GDFN — FeedForward.forward / backward (Restormer.py:76-93; moce_ir.py:255-276;
 * AdaIR-main/net/model.py:76-94).  hidden = h (project_in has 2h outputs).
 * ------------------------------------------------------------------------ */
/* flags bit 0: the forward also stores the depthwise conv's output for backward (no recompute; chosen by the caller and
 * passed unchanged to mi_gdfn_saved_bytes / _fwd / _bwd of one forward-backward pair: it fixes the saved blob's layout) */
typedef struct { int B, C, hidden, H, W, dtype, ks, flags; } mi_gdfn_shape;
typedef struct {
  const float* in_w;  const float* in_b;   /* [2h,C], [2h]|NULL */
  const float* dw_w;  const float* dw_b;   /* [2h,ks*ks], [2h]|NULL */
  const float* out_w; const float* out_b;  /* [C,h], [C]|NULL */
} mi_gdfn_params;
typedef struct { float* in_w; float* in_b; float* dw_w; float* dw_b; float* out_w; float* out_b; int accumulate; } mi_gdfn_grads;
size_t mi_gdfn_saved_bytes(const mi_gdfn_shape* s);
size_t mi_gdfn_workspace(const mi_gdfn_shape* s);
int mi_gdfn_fwd(const mi_gdfn_shape* s, const mi_gdfn_params* p, const void* x, const void* residual,
                void* out, void* saved, void* ws, void* stream);
int mi_gdfn_bwd(const mi_gdfn_shape* s, const mi_gdfn_params* p, const void* x, const void* dout,
                void* dx, const mi_gdfn_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * Fused GDFN half-block (bf16 activations):  out = y + FeedForward(LayerNorm(y))
 * = the second half of TransformerBlock.forward (Restormer.py:148 `x = x + self.ffn(self.norm2(x))`;
 * moce_ir.py:834 EncoderBlock; AdaIR-main/net/model.py:170) as ONE kernel: y is read once (plus a
 * one-pixel halo), out is written once; LN output, project_in output, conv outputs and the gate never
 * reach HBM.  Covered shapes (mi_gdfn_fused_ok): 3x3 depthwise, W % 64 == 0, H % 8 == 0, C = 48 or 96;
 * any hidden size.  Other shapes use mi_ln_fwd + mi_gdfn_fwd.
 *   mi_gdfn_fused_pack : LayerNorm weight/bias + the six GDFN parameters -> the kernel's packed bf16/fp32
 *                        weight images (LN affine folded into project_in).  Re-run after every weight update.
 *   mi_gdfn_fused_fwd  : y, out [B,C,H,W] bf16; mean/rstd [B,H*W] fp32 (both or neither; LN statistics of y
 *                        for the backward pass).
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, hidden, H, W, ln_with_bias; } mi_gdfn_fused_shape;
int mi_gdfn_fused_ok(const mi_gdfn_fused_shape* s);
size_t mi_gdfn_fused_pack_bytes(const mi_gdfn_fused_shape* s);
int mi_gdfn_fused_pack(const mi_gdfn_fused_shape* s, const float* ln_w, const float* ln_b, const mi_gdfn_params* p,
                       void* pack, void* stream);
int mi_gdfn_fused_fwd(const mi_gdfn_fused_shape* s, const void* pack, const void* y, void* out, float* mean,
                      float* rstd, void* stream);
/* Training form of the same launch: besides out and the statistics it writes what mi_gdfn_bwd / mi_gdfn_bwd_ln read - the
 * project_in output h0 [B,2h,H,W] and the gate output g [B,h,H,W] - into `saved`, a blob of mi_gdfn_saved_bytes() bytes for
 * the mi_gdfn_shape {B, C, hidden, H, W, MI_BF16, 3, flags 0}: the forward of `x + ffn(norm2(x))` (Restormer.py:148) is ONE
 * launch (10 C planes per pixel at hidden = 2.66 C) instead of GEMM -> depthwise gate -> GEMM (19).  _ok: covered shape. */
int mi_gdfn_fused_fwd_train_ok(const mi_gdfn_fused_shape* s);
int mi_gdfn_fused_fwd_train(const mi_gdfn_fused_shape* s, const void* pack, const void* y, void* out, float* mean,
                            float* rstd, void* saved, void* stream);
/* What the fused GDFN forwards launch for this shape under the current MI_FG_CFG / MI_FG_NOXCD (host-only).  entry: 0
 * mi_gdfn_fused_fwd, 1 mi_gdfn_fused_fwd_train, 2 mi_gdfn_fused_fwd_f8.  out[20]: covered, family (0 tile form / 1 fourth form),
 * C, tile rows TH, tile columns TW, gate pairs per chunk PC, waves, SAVE, F8, chunks of PC pairs (tile form), groups of two
 * 16-pair chunks (fourth form), tiles_x, tiles_y, workgroups per image S (tile form: one per tile; fourth form: persistent tile
 * ranges), grid (= B * S), block, dynamic LDS bytes, xcd_pairs (tile relabelling on), pack bytes, and the chunk width
 * mi_gdfn_fused_pack builds the tile sections of the pack for.  A pack built under one chunk width and run under another gives
 * wrong numbers without an error: pack and run under the same MI_FG_CFG.  An entry with no kernel instance for this shape and
 * these switches returns 0 with covered = 0 and every other field 0 (the launcher returns -1, mi_gdfn_fused_ok /
 * mi_gdfn_fused_fwd_train_ok say 0); -1 on a null pointer, a bad entry or a non-positive extent. */
int mi_gdfn_fused_plan(const mi_gdfn_fused_shape* s, int entry, int64_t* out);

/* ------------------------------------------------------------------------
 * Backward tail of a half-block  out = x + F(LN(x)),  F starting in the 1x1 conv h = W LN(x)
 * (TransformerBlock.forward, Restormer.py:146-150; qkv :105,115; project_in :82,89; WithBias_LayerNorm :52-64).
 * One launch computes, from dY = dL/dh:  dW += / = dY LN(x)^T,  dxn = W^T dY,  dx = LNbackward(dxn) + dres,
 * dgamma, dbeta - dY, x and dres are read once, dx written once; LN(x) is rebuilt from x and the saved statistics.
 * bf16 activations, C in {48, 96}, M <= 256 (C = 48) / 512 (C = 96), H*W a multiple of 64.
 *   mi_bwd_tail        : the kernel by itself.  dy [B,M,N], x (LayerNorm INPUT) / dres / dx [B,C,N], mean/rstd [B,N],
 *                        w [M,C], gamma/beta [C]; dw [M,C], dgamma, dbeta [C] (accumulate: += instead of =).
 *   mi_mdta_bwd_ln, mi_gdfn_bwd_ln : mi_mdta_bwd / mi_gdfn_bwd with that tail: x is the LayerNorm INPUT, dx the gradient of
 *                        the half-block's input; workspace from mi_*_bwd_ln_workspace (0 = shape not covered, see *_ok).
 * ------------------------------------------------------------------------ */
typedef struct {
  const float* w; const float* b;        /* LayerNorm weight, bias [C] */
  const float* mean; const float* rstd;  /* [B, H*W], from mi_ln_fwd */
  const void* dres;                      /* [B,C,H,W] gradient arriving over the residual connection, or NULL */
  float* dw; float* db;                  /* LayerNorm parameter gradients [C] */
} mi_ln_tail;
/* LayerNorm in front of the half-block's first 1x1 conv, applied inside that GEMM (the normalised tensor never reaches HBM):
 * mi_mdta_fwd_ln / mi_gdfn_fwd_ln = mi_mdta_fwd / mi_gdfn_fwd with x the LayerNorm INPUT.  mean / rstd [B, H*W] receive the
 * statistics for the backward pass (both or neither).  Shapes: mi_*_fwd_ln_ok (bf16, C <= 128, H*W a multiple of 64). */
typedef struct { const float* w; const float* b; float* mean; float* rstd; int with_bias; } mi_ln_head;
int mi_mdta_fwd_ln_ok(const mi_mdta_shape* s);
int mi_mdta_fwd_ln(const mi_mdta_shape* s, const mi_mdta_params* p, const mi_ln_head* ln, const void* x, const void* residual,
                   void* out, void* saved, void* ws, void* stream);
int mi_gdfn_fwd_ln_ok(const mi_gdfn_shape* s);
int mi_gdfn_fwd_ln(const mi_gdfn_shape* s, const mi_gdfn_params* p, const mi_ln_head* ln, const void* x, const void* residual,
                   void* out, void* saved, void* ws, void* stream);
/* fp8 (e4m3) MFMA operands in both 1x1 projections of a half-block - inference only (nothing is saved), bf16 activations in
 * HBM; see mi_pw_desc.f8.  x1 / w1 scale the first projection's input and weight (qkv: Restormer.py:105,114; project_in:
 * :82,89), x2 / w2 the second's (project_out, :107,131 - for MDTA its input is v and its weight the per-image product
 * project_out . softmax(..), |entries| <= (C / heads) max|project_out|; :86,92 for GDFN, input gelu(x1) x2).  Powers of two
 * with |operand| / scale <= 448 (values past that saturate).  ln may be NULL (x is then the LayerNorm output).
 * Shapes: mi_*_fwd_f8_ok(shape, with_ln). */
typedef struct { float x1, w1, x2, w2; } mi_f8_scales;
int mi_mdta_fwd_f8_ok(const mi_mdta_shape* s, int with_ln);
int mi_mdta_fwd_f8(const mi_mdta_shape* s, const mi_mdta_params* p, const mi_ln_head* ln, const mi_f8_scales* f8, const void* x,
                   const void* residual, void* out, void* ws, void* stream);
int mi_gdfn_fwd_f8_ok(const mi_gdfn_shape* s, int with_ln);
int mi_gdfn_fwd_f8(const mi_gdfn_shape* s, const mi_gdfn_params* p, const mi_ln_head* ln, const mi_f8_scales* f8, const void* x,
                   const void* residual, void* out, void* ws, void* stream);
/* mi_gdfn_fused_fwd (the one-launch LayerNorm + GDFN half-block) on fp8 operands: x1 scales the NORMALISED input
 * ((y - mu) rstd, |.| <= sqrt(C)) and w1 the packed W_in . diag(gamma); x2 / w2 as above.  Default tile forms only. */
int mi_gdfn_fused_fwd_f8(const mi_gdfn_fused_shape* s, const void* pack, const mi_f8_scales* f8, const void* y, void* out,
                         void* stream);

/* ------------------------------------------------------------------------
 * Fused MDTA, pass A (csrc/fused_mdta.hip; Restormer.py:111-122): LayerNorm -> qkv 1x1 -> depthwise 3x3 -> q k^T partials
 * + row sums of squares + v in ONE launch - x is read once, only v is written; qkv0, q and k never reach HBM.  mi_mdta_fused_fwd
 * runs the whole half-block on it: pass A, the fixed-order sum of the per-workgroup partials, the c x c softmax / W_o fold and
 * the per-image-weight GEMM  out = (W_o . blockdiag(A)) v (+ proj bias) (+ residual).  bf16, 3x3, C = 48 (1 head) or
 * 96 (1 or 2 heads), W % 64 == 0, H % 8 == 0 (mi_mdta_fused_ok); nothing is saved for backward (the no_grad path).
 *  pack : mi_mdta_fused_pack_bytes() bytes, written by mi_mdta_fused_pack from the LayerNorm affine (folded into W_qkv), the
 *         qkv / depthwise weights and biases; re-pack after every weight update.
 *  ln_with_bias : 1 WithBias ((x - mu) rstd), 0 BiasFree (x rstd, not centred).   mean / rstd : optional [B][H*W] outputs.
 *  ws   : mi_mdta_fused_workspace() bytes (v, the partials, the c x c matrices).
 * ------------------------------------------------------------------------ */
int mi_mdta_fused_ok(const mi_mdta_shape* s);
int mi_mdta_fused_pays(const mi_mdta_shape* s);   /* covered and enough workgroups (B x splits >= 192) to beat the unfused chain */
size_t mi_mdta_fused_pack_bytes(const mi_mdta_shape* s);
int mi_mdta_fused_pack(const mi_mdta_shape* s, const float* ln_w, const float* ln_b, const mi_mdta_params* p, void* pack,
                       void* stream);
size_t mi_mdta_fused_workspace(const mi_mdta_shape* s);
/* What pass A of mi_mdta_fused_fwd launches for this shape under the current MI_FM_CFG (host-only).  out[16]: covered, pays,
 * kind (1: C 48 one head, 2: C 96 two heads, 3: C 96 one head), form (0 round-3 / 1 fourth), tile rows TH, tiles_x, tiles_y,
 * persistent workgroups per image S, grid (= B * S), block, dynamic LDS bytes, part_mult (Gram partials a workgroup writes),
 * bytes of the partials' arena, workspace bytes, pack bytes, waves.  A shape the kernel does not cover returns 0 with
 * covered = 0 and every other field 0; -1 on a null pointer or a non-positive extent. */
int mi_mdta_fused_plan(const mi_mdta_shape* s, int64_t* out);
int mi_mdta_fused_fwd(const mi_mdta_shape* s, const mi_mdta_params* p, const void* pack, int ln_with_bias, const void* x,
                      const void* residual, void* out, float* mean, float* rstd, void* ws, void* stream);
/* ------------------------------------------------------------------------
 * The c x c side of MDTA by itself (csrc/attn_small.hip), c = C / heads in 1..128, Z = B * heads, everything fp32:
 *   fwd : graw [Z,c,c] = q k^T and ss [Z,2c] = (|q_i|^2, |k_j|^2) over the pixels, temperature [heads], wo [C,C] ->
 *         nrm [Z,2c] = max(sqrt(ss), 1e-12), P = graw / (|q_i||k_j|), A = softmax_row(temperature P) [Z,c,c], and the fold
 *         M [B,C,C], M[b][:, head cols] = wo[:, head cols] A, with bf16 copies Mb = M and Mtb = M^T per image (each may be NULL).
 *   bwd : dM [B,C,C] and the forward's A, P, nrm -> dwo_part [B,C,C] (its sum over images is dW_o), dtemp_part [Z] (its sum over
 *         images is d temperature) and wd [Z,2c,2c] = [[G1, diag D1], [diag D2, G1^T]], which maps the stacked [k; q] to
 *         [dq; dk]; wdb is its bf16 copy (may be NULL).
 * mi_attn_small_plan (host-only) reports what both launch.  out[16]: kernel instance CT (1, 2, 3, 4, 6, 8), promoted (ceil(c/16)
 * of 5 or 7 runs CT 6 or 8), padded width 16 CT, W_o row chunks of 16 per fold workgroup, fold grid x, fold grid y, chunks in
 * the last row group, fold LDS bytes, fold raises the 64 KiB LDS limit, backward grid x, backward grid y, backward LDS bytes,
 * backward raises the limit, row blocks of dA per wave, Mtb stored as vectors (C % 4 == 0), wd / wdb stored as vectors
 * (c % 4 == 0).  All three return -1 on a null pointer, B, C, heads <= 0, C % heads != 0 or c > 128.
 * ------------------------------------------------------------------------ */
int mi_attn_small_plan(int B, int C, int heads, int64_t* out);
int mi_attn_small_fwd(const float* graw, const float* ss, const float* temperature, const float* wo, float* P, float* A,
                      float* nrm, float* M, void* Mb, void* Mtb, int B, int C, int heads, void* stream);
int mi_attn_small_bwd(const float* dM, const float* A, const float* P, const float* nrm, const float* temperature,
                      const float* wo, float* dwo_part, float* dtemp_part, float* wd, void* wdb, int B, int C, int heads,
                      void* stream);
int mi_bwd_tail_ok(int M, int C, int64_t N, int dtype);
size_t mi_bwd_tail_workspace(int M, int C);
/* What mi_bwd_tail launches for this call under the current MI_BT_WIDE (host-only).  out[12]: covered, pays (covered and
 * faster than the unfused chain), waves per workgroup, 16-row fragments per wave, rows per wave, rows the workgroup holds,
 * workgroups launched, 64-pixel tiles, passes of the persistent loop, waves that hold rows, dynamic LDS bytes, workspace
 * bytes.  A shape the kernel does not cover returns 0 with covered = 0 and every other field 0; -1 on a null out, a bad dtype
 * code or M, B, N <= 0. */
int mi_bwd_tail_plan(int M, int C, int B, int64_t N, int dtype, int64_t* out);
int mi_bwd_tail(const void* dy, int M, const void* x, int C, const void* dres, const float* mean, const float* rstd,
                const float* w, const float* gamma, const float* beta, void* dx, float* dw, float* dgamma, float* dbeta,
                int B, int64_t N, int accumulate, int dtype, void* ws, void* stream);
int mi_mdta_bwd_ln_ok(const mi_mdta_shape* s, int qkv_bias);
size_t mi_mdta_bwd_ln_workspace(const mi_mdta_shape* s);
int mi_mdta_bwd_ln(const mi_mdta_shape* s, const mi_mdta_params* p, const mi_ln_tail* ln, const void* x, const void* dout,
                   void* dx, const mi_mdta_grads* gr, const void* saved, void* ws, void* stream);
int mi_gdfn_bwd_ln_ok(const mi_gdfn_shape* s, int in_bias);
size_t mi_gdfn_bwd_ln_workspace(const mi_gdfn_shape* s);
int mi_gdfn_bwd_ln(const mi_gdfn_shape* s, const mi_gdfn_params* p, const mi_ln_tail* ln, const void* x, const void* dout,
                   void* dx, const mi_gdfn_grads* gr, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * AdaIR frequency modules (AdaIR-main/net/model.py:230-372): the pieces of SpatialGate / ChannelGate / FreRefine / FreModule
 * that are not a block, a cross attention or a convolution (csrc/adair.hip).  Activations [B,C,H,W] in `dtype`, N = H*W.
 *   mi_box_down          F.interpolate(img, (H, W), 'bilinear') for the integer factors of the U-Net levels (model.py:321)
 *   mi_fre_rect          half sizes [B,2] of the low-frequency rectangle: int(h/n * sigmoid(rate_conv(avgpool))) (model.py:346-353)
 *   mi_fre_split_fwd/bwd FreModule.fft (model.py:343-372): high = |x - Px|, low = |Px|, P = the projection on the rectangle's
 *                        frequencies evaluated as a direct DFT (no FFT); half == NULL: empty rectangle for every sample.
 *                        coef: mi_fre_split_coef_bytes (kept for the backward); ws: mi_fre_split_workspace.
 *   mi_chan_maxmean_*    [max_c x, mean_c x] -> [B,2,H,W] + arg max [B,N] (model.py:240-242)
 *   mi_plane_max_fwd     global max pool + arg max per plane; mi_pool_pair_bwd: gradient of avg pool + max pool in one pass (model.py:250-264)
 *   mi_chan_gate_*       sigmoid(mlp(avg) + mlp(max)), mlp = W2 relu(W1 .) (model.py:253-268); hid [B,2,R] pre-activations
 *   mi_refine_mix_*      low * sigmoid(s0 + s1) + high * cw (model.py:284-288), s [B,2,H,W] = depthwise 7x7 of the max/mean planes
 *   mi_scale_add_*       a * p1[c] + y * p2[c] (model.py:331) and the parameter gradients
 * ------------------------------------------------------------------------ */
int mi_box_down(const void* img, void* out, int B, int C, int Hi, int Wi, int factor, int dtype, void* stream);
int mi_fre_rect(const float* pooled, const float* w0, const float* w2, int* half, int B, int C, int R, int H, int W, int n,
                void* stream);
size_t mi_fre_split_coef_bytes(int B, int C);
size_t mi_fre_split_workspace(int B, int C, int H, int W);
int mi_fre_split_max_hw(void);
int mi_fre_split_fwd(const void* feat, const int* half, void* high, void* low, float* coef, int B, int C, int H, int W, int dtype,
                     void* stream);
int mi_fre_split_bwd(const void* feat, const int* half, const float* coef, const void* dhigh, const void* dlow, void* dfeat, int B,
                     int C, int H, int W, int dtype, void* ws, void* stream);
int mi_chan_maxmean_fwd(const void* x, void* out, int* idx, int B, int C, int64_t N, int dtype, void* stream);
int mi_chan_maxmean_bwd(const void* dout, const int* idx, void* dx, int B, int C, int64_t N, int dtype, void* stream);
int mi_plane_max_fwd(const void* x, float* out, int* idx, int planes, int64_t N, int dtype, void* stream);
int mi_pool_pair_bwd(const float* davg, const float* dmax, const int* idx, void* dx, int planes, int64_t N, int dtype, void* stream);
int mi_chan_gate_fwd(const float* avg, const float* mx, const float* w1, const float* w2, float* cw, float* hid, int B, int C, int R,
                     void* stream);
int mi_chan_gate_bwd(const float* avg, const float* mx, const float* w1, const float* w2, const float* cw, const float* hid,
                     const float* dcw, float* davg, float* dmx, float* dw1, float* dw2, int B, int C, int R, int accumulate,
                     void* stream);
int mi_refine_mix_fwd(const void* low, const void* high, const void* s, const float* cw, void* out, int B, int C, int64_t N,
                      int dtype, void* stream);
int mi_refine_mix_bwd(const void* low, const void* high, const void* s, const float* cw, const void* dout, void* dlow, void* dhigh,
                      void* ds, float* dcw, int B, int C, int64_t N, int dtype, void* stream);
int mi_scale_add_fwd(const void* a, const void* y, const float* p1, const float* p2, void* out, int B, int C, int64_t N, int dtype,
                     void* stream);
int mi_scale_add_bwd(const void* a, const void* y, const float* p1, const float* p2, const void* dout, void* da, void* dy, float* dp1,
                     float* dp2, int B, int C, int64_t N, int accumulate, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Training-step tail on flat fp32 buffers (MoCE-IR-main/src/train.py:79-88:
 * AdamW(lr=2e-4), torch defaults betas (0.9,0.999), eps 1e-8, weight_decay 1e-2).
 * p, g, m, v: [n] fp32.  grad_scale multiplies g first (1/world for DDP mean).
 * dev_scalars (device, may be NULL): {lr, 1-beta1^step, sqrt(1-beta2^step)} read by the kernel
 * instead of the host lr/step, so that a captured HIP graph can be replayed with new values.
 * ------------------------------------------------------------------------ */
int mi_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale,
                  const float* dev_scalars, void* stream);

/* Gradient-norm clipping and weight EMA (BasicSR image_restoration_model.py: use_grad_clip ->
 * clip_grad_norm_(params, 0.01); ema_decay -> model_ema, saved as params_ema).
 * grad_sumsq: *out = sum x[i]^2 over [n] fp32 (x 16-byte aligned), written to device memory.
 *   Two launches with a fixed grid per n and a fixed order (bitwise reproducible), fp64 accumulation.
 *   workspace: caller-owned device buffer of mi_grad_sumsq_workspace(n) bytes (<= 8 KiB).
 * adamw_step_ex: mi_adamw_step plus, when sumsq != NULL (device scalar, e.g. from mi_grad_sumsq),
 *   norm = sqrt(*sumsq) * grad_scale, coef = min(max_norm / (norm + 1e-6), 1) (torch clip_grad_norm_,
 *   error_if_nonfinite=False: inf / NaN propagate), gradient (g * grad_scale) * coef; norm_out (device,
 *   may be NULL) receives norm.  When ema != NULL ([n] fp32), after the update
 *   ema = ema * ema_decay + p * (1 - ema_decay).  Nothing is read back to the host: graph capture works.
 *   With sumsq == NULL and ema == NULL it computes bitwise what mi_adamw_step does.
 * ------------------------------------------------------------------------ */
size_t mi_grad_sumsq_workspace(int64_t n);
int mi_grad_sumsq(const float* x, int64_t n, float* out, void* workspace, void* stream);
int mi_adamw_step_ex(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                     const float* dev_scalars, const float* sumsq, float max_norm, float* norm_out,
                     float ema_decay, void* stream);

/* ------------------------------------------------------------------------
 * MoCE SparseDispatcher data movement (moce_ir.py:71-143).  A "row" is one sample's feature map (C*H*W elements);
 * idx is the dispatcher's _batch_index (int64, device), scale its _nonzero_gates (fp32, device).
 *   rows_gather      : out[i] = x[idx[i]]                                    (dispatch, :103)
 *   rows_scatter_add : out[b] = sum_{i: idx[i]==b} scale[i] * src[i]          (combine: gate multiply + index_add into
 *                      zeros, fp32 accumulation, :116-124; scale NULL = 1; out is fp32 or the activation dtype)
 *   rows_gather_scaled: out[i] = scale[i] * x[idx[i]], fp32 x -> activation dtype (gradient of combine w.r.t. expert outputs)
 *   rows_dot         : out[i] = <g[idx[i]], src[i]>                           (gradient of the gate values)
 * The scatter is per destination row in list order: deterministic, no atomics.
 * ------------------------------------------------------------------------ */
int mi_rows_gather(const void* x, const int64_t* idx, void* out, int n_out, int64_t row, int dtype, void* stream);
int mi_rows_gather_scaled(const float* x, const int64_t* idx, const float* scale, void* out, int n_out, int64_t row,
                          int out_dtype, void* stream);
int mi_rows_scatter_add(const void* src, const int64_t* idx, const float* scale, void* out, int n_src, int n_rows,
                        int64_t row, int dtype, int out_f32, void* stream);
size_t mi_rows_dot_workspace(int n_src, int64_t row);
int mi_rows_dot(const float* g, const void* src, const int64_t* idx, float* out, int n_src, int64_t row, int dtype,
                void* ws, void* stream);

/* ------------------------------------------------------------------------
 * Grouped expert GEMM (csrc/grouped.hip): the 1x1 projections of all MoCE experts in ONE launch over a problem table whose
 * ragged part - rows per expert, segment starts - is read from DEVICE memory (the router's counts / offsets tables), so no
 * segment size has to reach the host for this stage.  Replaces the per-expert 1x1 calls of moce_ir.py:545-558 (ModExpert.process:
 * proj[0], proj[1], proj[2]) as iterated by :666-672, whose split sizes the reference reads back with .tolist() (:88).
 *   for every problem p, for i in [0, counts[p.expert]):
 *       Y_p[row_y] = W_p . X_p[row_x] (+ bias_p) (+ R_p[row_r]),   row_* = i (local) or offsets[p.expert] + i (stitched buffers)
 *   X rows are [K][N], Y / R rows [M][N] (N = H*W pixels, contiguous); W element (m, k) at w[m*w_sm + k*w_sk] (fp32; a
 *   transposed use - the input gradient W^T dY - is just swapped strides); *_rs row strides in elements (0 = dense).
 * Up to 16 problems per launch; the grid covers max_rows rows per problem, workgroups beyond an expert's count exit at once.
 * ------------------------------------------------------------------------ */
typedef struct {
  const void* x; int64_t x_rs;
  const float* w; int64_t w_sm, w_sk;
  const float* bias;
  const void* r; int64_t r_rs;
  void* y; int64_t y_rs;
  int m, k;
  int expert;                     /* index into dev_counts / dev_offsets */
  int x_local, y_local, r_local;  /* 1: the buffer is indexed by the row's position inside the expert's segment */
} mi_grouped_problem;
int mi_grouped_pw_gemm(const mi_grouped_problem* probs, int np, const int* dev_counts, const int* dev_offsets, int max_rows,
                       int64_t N, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * MoCE router in one launch each way (moce_ir.py:684-800 RoutingFunction; :82-91 SparseDispatcher index bookkeeping).
 *   fwd: logits = pooled . Wg^T + freq . Wf^T  (pooled = GAP of the adapter input, [B,C]; freq = frequency embedding [B,F]);
 *        noisy = logits + noise / E  (noise: the caller's N(0,1) draw, [B,E], applied in train AND eval as the reference does);
 *        scores = softmax(noisy); top-k -> topk_idx [B,k] (int64), topk_val [B,k]; gates [B,E] = scores scattered at the top-k;
 *        aux[0] = 0.5 CV^2(sum_b softmax(logits) * complexity) + 0.5 CV^2(mean_b (1 - Phi((thr_b - logits) * E)))  when
 *        training != 0 (complexity may be NULL = no complexity bias), else 0;
 *        dispatch tables: counts[E], offsets[E+1], and for the B*k dispatched rows grouped by expert (samples ascending within
 *        an expert): perm (sample index, int64), perm_gate (its gate value), perm_expert; row_of [B,k] = the dispatched row
 *        of sample b's j-th choice.
 *   bwd: given dgates [B,E] (may be NULL), drow [B*k] (gradient of perm_gate, may be NULL) and daux (device scalar, may be
 *        NULL): dpooled [B,C], dfreq [B,F], dwg [E,C], dwf [E,F] (overwritten).  E <= 8, B*E <= 8192.
 * ------------------------------------------------------------------------ */
int mi_moe_route_fwd(const float* pooled, const float* freq, const float* wg, const float* wf, const float* noise,
                     const float* complexity, float* logits, float* gates, int64_t* topk_idx, float* topk_val, float* aux,
                     int* counts, int* offsets, int64_t* perm, float* perm_gate, int* perm_expert, int* row_of, int B, int C, int F,
                     int E, int k, int training, void* stream);
int mi_moe_route_bwd(const float* pooled, const float* freq, const float* wg, const float* wf, const float* noise,
                     const float* complexity, const float* logits, const int64_t* topk_idx, const float* dgates,
                     const float* drow, const int* row_of, const float* daux, float* dpooled, float* dfreq, float* dwg, float* dwf,
                     int B, int C, int F, int E, int k, int training, void* stream);

/* ------------------------------------------------------------------------
 * FFTAttention's patch spectrum product (moce_ir.py:408-414): irfft2(rfft2(x) * rfft2(y)) over every patch x patch block of
 * each [H,W] plane = the 2-D circular convolution  out[u][v] = sum_{a,b} x[a][b] y[(u-a)%p][(v-b)%p], evaluated directly in
 * fp32 from/to NCHW planes (zero padded to the patch grid at the bottom/right edge, cropped back; patch in {4,8,16,32}).
 * flip != 0 uses y'[i][j] = y[-i][-j]: dx = circconv(dout, y, flip=1), dy = circconv(dout, x, flip=1).
 * x_bs / y_bs / out_bs: batch strides in elements (0 = C*H*W), so that channel slices of a wider tensor (k of kv, the
 * k half of d_kv) need no copy.
 * ------------------------------------------------------------------------ */
int mi_patch_circconv(const void* x, int64_t x_bs, const void* y, int64_t y_bs, void* out, int64_t out_bs, int B, int C, int H,
                      int W, int patch, int flip, int dtype, void* stream);

/* FrequencyEmbedding's GELU -> spatial mean (moce_ir.py:1062-1064,1071-1073): out[b,c] = mean_n gelu(x[b,c,n]) (fp32);
 * bwd: dx = dout[b,c]/N * gelu'(x). */
int mi_gelu_gap_fwd(const void* x, float* out, int B, int C, int64_t N, int dtype, void* stream);
int mi_gelu_gap_bwd(const void* x, const float* dout, void* dx, int B, int C, int64_t N, int dtype, void* stream);

/* Gating products of the expert path: op 0  out = a * b  (FFTAttention `out * v`, moce_ir.py:419);
 * op 1  out = a * silu(b)  (ModExpert `body(x) * silu(proj[1](shared))`, :555);  op 2  out = gelu_erf(a), b unused
 * (FrequencyEmbedding's MLP activation, :1071).  bwd writes da and db (op 2: da only). */
/* a, b (and da, db) are [rows][L] with row strides in elements (0 = L); out and dout are contiguous [rows][L]. */
int mi_ewise_fwd(const void* a, int64_t a_rs, const void* b, int64_t b_rs, void* out, int64_t rows, int64_t L, int op, int dtype,
                 void* stream);
int mi_ewise_bwd(const void* a, int64_t a_rs, const void* b, int64_t b_rs, const void* dout, void* da, int64_t da_rs, void* db,
                 int64_t db_rs, int64_t rows, int64_t L, int op, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * U-Net glue, thin dense 3x3 convolutions (Restormer.py:156-165 OverlapPatchEmbed 3->48; :243,281 output conv 2*dim->3
 * + input residual).  Layout kernels that turn them into the 1x1 GEMM / Gram above:
 *   im2col3x3: x[B,C,H,W] -> col[B,9C,H,W], col[c*9+ky*3+kx][y][x] = x[c][y+ky-1][x+kx-1] (zero padded);
 *              flip != 0 negates the shifts (the im2col of the transposed convolution).
 *   col2im3x3: z[B,9M,H,W] -> y[B,M,H,W],  y[m][y][x] = sum_taps z[m*9+ky*3+kx][y+ky-1][x+kx-1] (+ bias[m]) (+ residual);
 *              flip != 0 negates the shifts (scatter of the transposed convolution: input gradient of the im2col form).
 * conv(x;W) = W[Cout,9Cin] . im2col(x) when Cin is tiny; = col2im(Wz[9Cout,Cin] . x) when Cout is tiny.
 * Any H, W: rows of 16..256 pixels (power of two) on 16-byte aligned planes take the wave-streaming forms, everything
 * else an element-wise general form (mi_glue3x3_ok: H, W >= 1).
 * ------------------------------------------------------------------------ */
int mi_glue3x3_ok(int H, int W);
int mi_im2col3x3(const void* x, void* out, int B, int C, int H, int W, int flip, int dtype, void* stream);
int mi_col2im3x3(const void* z, const float* bias, const void* residual, void* y, int B, int M, int H, int W, int flip,
                 int dtype, void* stream);
/* What mi_im2col3x3 / mi_col2im3x3 launch for `planes` planes (B * C, B * M) of H x W (host-only; the launchers decide by the
 * same code); aligned: whether every activation pointer of the call lies on a 16-byte boundary.  out[6]: fast (1 = the
 * wave-streaming form: W in {16,32,64,128,256} and aligned; 0 = the element-wise general form), lpr (lanes per row = W / 4:
 * 4..64; 0 in the general form), band (rows a lane group walks: 8, or 16 / 32 when that still leaves >= 4096 waves; 0 in the
 * general form), bands per plane, blocks of the im2col grid, blocks of the col2im grid (general form: one thread per output
 * element, capped at 65536 blocks of a grid-stride loop).  -1 on a null out, a bad dtype code, planes < 1 or H, W < 1. */
int mi_glue3x3_plan(int64_t planes, int H, int W, int dtype, int aligned, int64_t* out);

/* ------------------------------------------------------------------------
 * Dense 3x3 convolution (stride 1, zero padding 1) as an implicit GEMM (csrc/conv3x3.hip): the glue convs above and the
 * C -> C/2 / C -> 2C bodies of Downsample / Upsample (Restormer.py:171-189) without the 9-plane im2col expansion in HBM.
 * bf16 activations, fp32 accumulate, W % 8 == 0 (mi_conv3x3_ok); other planes / fp32 use the im2col forms above.
 *   mi_conv3x3_pack : w fp32 -> the kernel's fragment-major bf16 image (mi_conv3x3_pack_bytes(M, K) bytes; re-pack after every
 *                     weight update).  transpose_flip == 0: w is [M][K][3][3] and the op is y = conv(x; w).
 *                     transpose_flip != 0: w is the conv's own weight [K][M][3][3] and the op is its DATA GRADIENT
 *                     dx[M planes] = conv_transpose(dy[K planes]; w)  (taps flipped, channel roles swapped).
 *   mi_conv3x3_fwd  : y[B,M,H,W] = conv(x[B,K,H,W]) (+ bias[m]) (+ residual[B,M,H,W]); x_bs / r_bs / y_bs batch strides in
 *                     elements (0 = dense) so operands may be channel slices; channel planes dense H*W.
 *   mi_conv3x3_wgrad: dw[M][K][3][3] (+)= sum_{b,p} dy[b][m][p] . x[b][k][p + d(tap)]; ws = mi_conv3x3_wgrad_workspace bytes.
 * ------------------------------------------------------------------------ */
int mi_conv3x3_ok(int H, int W, int dtype);
size_t mi_conv3x3_pack_bytes(int M, int K);
int mi_conv3x3_pack(const float* w, int M, int K, int transpose_flip, void* pack, void* stream);
int mi_conv3x3_fwd(const void* pack, const void* x, int64_t x_bs, const float* bias, const void* residual, int64_t r_bs,
                   void* y, int64_t y_bs, int B, int M, int K, int H, int W, void* stream);
size_t mi_conv3x3_wgrad_workspace(int B, int M, int K, int H, int W);
int mi_conv3x3_wgrad(const void* dy, int64_t dy_bs, const void* x, int64_t x_bs, float* dw, int accumulate, int B, int M, int K,
                     int H, int W, void* ws, void* stream);
/* What the three kernels launch for y[B,M,H,W] = conv(x[B,K,H,W]) (host-only; the launchers decide by the same code).  out[15]:
 *   forward / data gradient (for the data gradient pass the op's own M and K: M = planes written, K = planes read):
 *     mt (16-row m-tiles per workgroup: 1 for M <= 16, 2 for M <= 32, else 4), twp (tile width: 16 for W <= 16, 32 for W <= 32,
 *     else 64), tr (tile rows = 256 / twp), tiles_x, tiles_y, co_tiles (grid.y = ceil(M / (16 mt))), chunks (16-channel chunks of
 *     K), pack_bytes (= mi_conv3x3_pack_bytes);
 *   weight gradient: w_swap (1: x takes the 64-row role and dy the 16-column role - the choice that pads less), w_rows, w_cols
 *     (the M and K the kernel sees after the swap), w_splits (workgroups that share the pixel tiles of one 64 x 16 block: split s
 *     takes tiles s, s + w_splits, ... of the B * tiles_x * tiles_y), w_grid_x (= ceil(w_cols / 16)), w_grid_y (= ceil(w_rows / 64)),
 *     w_workspace (= mi_conv3x3_wgrad_workspace).
 * -1 on a null out, B, M, K < 1 or a plane mi_conv3x3_ok refuses. */
int mi_conv3x3_plan(int B, int M, int K, int H, int W, int64_t* out);

/* PixelShuffle(2) / PixelUnshuffle(2) of Upsample / Downsample (Restormer.py:171-189; moce_ir.py Downsample/Upsample):
 *   unshuffle == 0: in [B,4c,H,W] -> out [B,c,2H,2W], out[b][c][2y+i][2x+j] = in[b][4c+2i+j][y][x]
 *   unshuffle != 0: in [B,c,2H,2W] -> out [B,4c,H,W] (the inverse; also each other's backward).
 * in_bs / out_bs: batch strides in elements (0 = dense), so the high-resolution side may be a channel slice of the decoder's
 * concatenation buffer (Restormer.py:266 torch.cat).  mi_copy_rows moves [rows][L] with row strides (the skip half of it). */
int mi_pixel_shuffle2(const void* in, int64_t in_bs, void* out, int64_t out_bs, int B, int c, int H, int W, int unshuffle,
                      int dtype, void* stream);
int mi_copy_rows(const void* src, int64_t src_rs, void* dst, int64_t dst_rs, int64_t rows, int64_t L, int dtype, void* stream);
/* What the two launch (host-only; the launchers decide by the same code); strides as in the calls (0 = dense), aligned: whether
 * both pointers lie on a 16-byte boundary.  out[3]: vector (elements per access: 16 bytes = 8 bf16 / 4 fp32 when W (L), both
 * strides and both pointers allow it, else 1 = the element-wise form), total (work items: B c 2 H (W / vector); rows (L /
 * vector)), blocks (ceil(total / 256), capped at 16384 blocks of a grid-stride loop).  -1 on a null out, a bad dtype code, a
 * non-positive extent or a negative stride. */
int mi_pixel_shuffle2_plan(int B, int c, int H, int W, int64_t in_bs, int64_t out_bs, int dtype, int aligned, int64_t* out);
int mi_copy_rows_plan(int64_t rows, int64_t L, int64_t src_rs, int64_t dst_rs, int dtype, int aligned, int64_t* out);

/* ------------------------------------------------------------------------
 * Router global average pool (moce_ir.py:703-707, RoutingFunction.gate[0]): out[b,c] = mean_n x[b,c,n] (fp32);
 * bwd: dx[b,c,:] = dout[b,c]/N.
 * ------------------------------------------------------------------------ */
int mi_gap_fwd(const void* x, float* out, int B, int C, int64_t N, int dtype, void* stream);
/* bias gradient of a conv (nn.Conv2d(bias=True)): out[c] (+)= sum over batch and pixels of x[b][c][n]; fixed summation order */
size_t mi_chan_sum_workspace(int C, int64_t N);
/* What mi_chan_sum launches for x [B,C,N] (host-only); aligned: whether the base pointer lies on a 16-byte boundary.  out[4]:
 * splits of the pixel axis, pixels per split (a multiple of 8; the last split ends at N), whether the kernel loads whole
 * 16-byte vectors (N a multiple of the vector and an aligned base), workspace bytes.  -1 on a null out, a bad dtype code or
 * B, C, N <= 0. */
int mi_chan_sum_plan(int B, int C, int64_t N, int dtype, int aligned, int64_t* out);
int mi_chan_sum(const void* x, float* out, int B, int C, int64_t N, int dtype, int accumulate, void* ws, void* stream);
int mi_gap_bwd(const float* dout, void* dx, int B, int C, int64_t N, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Training samples on the device (MoCE-IR-main/src/data/dataset_utils.py:156-165 AIOTrainDataset.__getitem__, denoise tasks;
 * src/data/degradation_utils.py:21-24; src/utils/image_utils.py data_augmentation): for sample b of the batch
 *   patch = image[sample[b]][top[b] : top[b]+P, left[b] : left[b]+P]      (decoded uint8 HWC images in one flat `pool`,
 *                                                                           image s at pool + src_off[s], src_h[s] x src_w[s])
 *   aug   = data_augmentation(patch, mode[b])                              (the 8 dihedral modes, numbered as the reference)
 *   clean[b]    = aug / 255                                                 (CHW, activation dtype)
 *   degraded[b] = uint8(clip(aug + sigma[b] * noise[b], 0, 255)) / 255      (noise: the caller's N(0,1) draw, [B,3,P,P])
 * clean or degraded may be NULL.  The caller keeps top/left inside the image.
 * ------------------------------------------------------------------------ */
int mi_patch_batch(const unsigned char* pool, const int64_t* src_off, const int* src_h, const int* src_w, const int* sample,
                   const int* top, const int* left, const int* mode, const float* sigma, const float* noise, void* clean,
                   void* degraded, int B, int P, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Evaluation metrics as the reference's test loops compute them through scikit-image (AdaIR-main/utils/val_utils.py:50-64;
 * MoCE-IR-main/src/test.py:82-123): inputs clipped to [0,1];  psnr[b] = 10 log10(1 / MSE);  ssim[b] = structural_similarity
 * with data_range 1, 7x7 uniform window, K1 0.01, K2 0.03, sample covariance, 3-pixel border excluded, channel mean.
 * ws: mi_psnr_ssim_workspace() bytes.  Deterministic (fixed-order sums).
 * ------------------------------------------------------------------------ */
size_t mi_psnr_ssim_workspace(int B, int C, int H, int W);
int mi_psnr_ssim(const void* restored, const void* clean, float* psnr, float* ssim, int B, int C, int H, int W, int dtype,
                 void* ws, void* stream);

/* dtype conversion / L1 loss helpers used by the harness */
int mi_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* loss[0] += mean|a-b| ; da = sign(a-b) * scale (da may be NULL); loss must hold 1+1024 floats
 * (entries 1.. are scratch for the block partials) */
int mi_l1_loss(const void* a, const void* b, void* da, float* loss, int64_t n, float scale, int dtype,
               void* stream);

/* ------------------------------------------------------------------------
 * FFT loss (MoCE-IR-main/src/utils/loss_utils.py:139-152) without an FFT library (csrc/fftloss.hip):
 *   loss[0] = loss_weight * mean(|Re Z| + |Im Z|),  Z = rfft2(pred - target) over the last two axes of [B,C,H,W]
 *   dpred   = d loss / d pred, written in `dtype` (rounded once from fp32); may be NULL (the adjoint stages are skipped).
 * The transform is a two-stage dense DFT on the fp32-input MFMA, fp32 throughout (inputs widened on load); the gradient is the
 * adjoint applied to sign(Re Z) + i sign(Im Z) on the half spectrum, sign(0) = 0.  2 <= H, W <= 512, any B*C >= 1; anything
 * else is refused.  Bitwise reproducible (no atomics, fixed-order sums).  loss: one device float, overwritten.
 * ws: mi_fft_l1_workspace() bytes (twiddle tables, intermediates and loss partials, all rebuilt each call).
 * mi_fft_l1_plan (host-only; the launcher takes every decision from the same plan) fills out[40]: planes B*C, K = W/2 + 1,
 * tile rows, contraction depth per LDS stage, l block width, l blocks, x block width, x blocks, 64-row tiles over B*C*H,
 * 64-row tiles over H, grid of the table fill, grids of stages 1..4 (0: not launched), threads per workgroup, loss partials,
 * launches of their sum, launches in all; then (byte offset, bytes) of the ten workspace sections cos W, sin W, cos W^T,
 * sin W^T, cos H, sin H, T (the gradient's gT reuses it), S, the partials, the sum's scratch; last, the workspace size.
 * ------------------------------------------------------------------------ */
size_t mi_fft_l1_workspace(int B, int C, int H, int W);
int mi_fft_l1_plan(int B, int C, int H, int W, int dtype, int want_grad, int64_t* out);
int mi_fft_l1_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                   float loss_weight, int dtype, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * The real 2-D transforms on their own and DarkIR's FreMLP (DarkIR-main/archs/arch_model.py:36-55), without an FFT library
 * (csrc/fremlp.hip): the dense-DFT GEMMs of the FFT loss, fp32 between the input load and the output store.  K = W/2 + 1.
 *   mi_dft2_r2c   x [B,C,H,W] in `dtype` -> Re Z, Im Z [B,C,H,K] fp32,  Z = rfft2(x):
 *                 Z[k,l] = sum_y sum_x x[y,x] exp(-2 pi i (k y / H + l x / W)).
 *   mi_dft2_c2r   Re Y, Im Y [B,C,H,K] fp32 -> out [B,C,H,W] in `dtype` (rounded once):
 *                 out[y,x] = 1/(HW) sum_l w_l Re( exp(+2 pi i l x / W) sum_k exp(+2 pi i k y / H) Y[k,l] ),
 *                 w_l = 1 at l = 0 and, for even W, at l = W/2 (odd W has no Nyquist column), 2 at every other l.  This IS
 *                 irfft2(Y, s=(H,W), norm='backward') for ANY Y: the imaginary parts that a c2r transform drops in the edge
 *                 columns are dropped here by the same formula; no Hermitian fix-up is needed or made.
 *   ws: mi_dft2_workspace() bytes serve both (twiddle tables and one complex intermediate, rebuilt each call).
 *
 *   FreMLP        Z = rfft2(x);  mag = sqrt(Re Z^2 + Im Z^2);  u = Z / mag, and u = (1, 0) where mag == 0 (torch.angle(0) = 0);
 *                 mag' = W2 LeakyReLU_0.1(W1 mag + b1) + b2 over the nc channels of each frequency bin
 *                 (W1 [expand nc, nc], W2 [nc, expand nc], both biases required);  out = irfft2(mag' u, s=(H,W)).
 *                 No atan2, cos or sin of data is taken.  x, out, dout, dx in `dtype` (widened on load, rounded once on store);
 *                 spectra, the MLP, the saved blob, parameters and their gradients fp32.
 *   backward      G = the adjoint of c2r applied to dout;  dmag' = G . u (real dot product),  du = mag' G;  the MLP backward
 *                 gives dmag, dW1, db1, dW2, db2;  dZ = dmag u + (du - u (u . du)) / mag, and dZ = 0 where mag == 0 (abs and
 *                 angle have zero gradient there);  dx = the adjoint of r2c applied to dZ (real, no column doubling).
 *                 accumulate: the four parameter gradients are added to (1) or overwritten (0), as in mi_dblock_bwd.
 *   saved         mi_fremlp_saved_bytes(): Z and the hidden activations, fp32 ((2 + expand) floats per bin and channel); mag, u
 *                 and mag' are recomputed.  saved == NULL in mi_fremlp_fwd: inference, nothing is kept.
 * Limits: 2 <= H, W <= 512 (larger images need tiling or a factored DFT: not built), 1 <= nc <= 256, expand >= 1 with
 * expand nc <= 512, any B >= 1 (B nc H K and B expand nc H K below 2^31).  Anything else is refused before any launch; the
 * sizing calls return 0.  Bitwise reproducible (no atomics, fixed-order sums).  No allocation, no host synchronisation.
 * mi_fremlp_plan (host-only; the launchers and the sizing calls read the same plan) fills out[64]: planes B nc, K, hidden width,
 * tile rows, contraction depth per LDS stage, l block width, l blocks, x block width, x blocks, 64-row tiles over B nc H, 64-row
 * tiles over H, grids of the table fill, of the [B nc H] x K stages, of the per-plane stages, of the [B nc H] x W stages, of the
 * per-bin passes, of the hidden passes, threads per workgroup, own kernel launches forward / backward, library calls (1x1
 * product, Gram, channel sum) forward / backward; then (byte offset, bytes) of the 19 workspace sections: cos W, sin W, their
 * transposes, the same four with w_l folded in, cos H, sin H, two complex intermediates, Z and the hidden plane (used when
 * nothing is saved; the hidden plane also holds the hidden gradient), two real planes, the 1x1 / Gram / channel-sum
 * workspaces [22..59]; the workspace size [60], the saved blob's size [61], the offset of the hidden activations in it [62]; 0.
 * ------------------------------------------------------------------------ */
typedef struct { int B, nc, expand, H, W, dtype; } mi_fremlp_shape;
size_t mi_dft2_workspace(int B, int C, int H, int W);
int mi_dft2_r2c(const void* x, float* zre, float* zim, int B, int C, int H, int W, int dtype, void* ws, void* stream);
int mi_dft2_c2r(const float* yre, const float* yim, void* out, int B, int C, int H, int W, int dtype, void* ws, void* stream);
size_t mi_fremlp_workspace(const mi_fremlp_shape* s);
size_t mi_fremlp_saved_bytes(const mi_fremlp_shape* s);
int mi_fremlp_plan(const mi_fremlp_shape* s, int64_t* out);
int mi_fremlp_fwd(const mi_fremlp_shape* s, const float* w1, const float* b1, const float* w2, const float* b2, const void* x,
                  void* out, void* saved, void* ws, void* stream);
int mi_fremlp_bwd(const mi_fremlp_shape* s, const float* w1, const float* w2, const float* b2, const void* dout, void* dx,
                  float* g_w1, float* g_b1, float* g_w2, float* g_b2, int accumulate, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * SFHformer's FourierUnit (SFHformer.py:143-180; csrc/sfh.hip): BatchNorm, a depthwise 3x3 with residual, a softmax gate over G
 * groups, a grouped 1x1 and GELU, all on the half spectrum between rfft2 and irfft2 (norm='ortho'), fp32 between the input load
 * and the output store.  c = in_channels = out_channels, C2 = 2c, K = W/2 + 1, S = C2 / G; the reference's interleaved spectral
 * channel j = 2i + d is Re Z_i (d = 0) / Im Z_i (d = 1): pure indexing on the planar spectra of mi_dft2_r2c, no copy is made.
 *   t1 = BatchNorm(Z / sqrt(HW))   bn_w, bn_b, running_mean, running_var [C2].  Training: the batch mean and biased variance over
 *        the B H K bins of each channel normalise, and running_mean <- (1 - momentum) rm + momentum mean, running_var <-
 *        (1 - momentum) rv + momentum var n / (n - 1), in place, on the device, in the same launch sequence (num_batches_tracked is
 *        the caller's).  Eval: the running statistics normalise, nothing is updated.  The ortho scale is folded in exactly: with
 *        mu, var of the unscaled Z,  xhat = (z - mu) alpha / sqrt(alpha^2 var + eps), alpha = 1 / sqrt(HW): eps is not rescaled.
 *        The variance is a fixed-order merge of per-chunk (mean, sum of squared deviations from that mean) pairs: no difference of
 *        large sums, no atomics.
 *   t  = fpe(t1) + t1              fpe_w [C2, 9], fpe_b [C2]: depthwise 3x3, zero padding 1, over the (H, K) plane
 *   s  = softmax_g(gate_w t + gate_b)   gate_w [G, C2], gate_b [G]  (the reference's `weight.0`)
 *   pre[k] = sum_j W'[k, j] s_{j / S} t[j] + sum_g s_g fdc_b[g C2 + k],  W'[k, g S + jl] = fdc_w[g C2 + k, jl]   (fdc_w [G C2, S]):
 *        the grouped 1x1 and the gate-weighted sum over groups as ONE C2 x C2 product on the gate-scaled input (mi_pw_gemm at
 *        fp32); the [B, G C2, H, K] tensor is never formed, forward or backward.
 *   out = irfft2(gelu_erf(pre), s=(H,W), norm='ortho')   (mi_dft2_c2r's formula: the parts irfft2 drops are dropped)
 *   backward   dx and all eight parameter gradients (added to when g->accumulate, else overwritten); BatchNorm's backward in the
 *        full training form (mean(dy), mean(dy xhat)) when `training`, the plain affine form otherwise.
 *   saved      mi_fourier_unit_saved_bytes(): Z (fp32, 2 floats per bin and channel) and the per-channel (mu, r); t, s, the gate-
 *        scaled input and pre are recomputed by the forward's own kernels.  saved == NULL in _fwd: inference or no_grad, nothing is
 *        kept (the running statistics are still updated when `training`).
 * Limits: 2 <= H, W <= 512, 1 <= c <= 256, 1 <= groups <= 8 with 2c % groups == 0 (c % groups != 0 is fine), fp32 or bf16,
 * B 2c H K below 2^31, eps > 0, 0 <= momentum <= 1.  Anything else is refused before any launch; the sizing calls return 0.
 * Bitwise reproducible (no atomics, fixed-order sums).  No allocation, no host synchronisation.
 * mi_fourier_unit_plan (host-only; the launchers and the sizing calls read the same plan) fills out[64]: planes B c, K, 2c, groups,
 * S, elements B 2c H K, bins B H K, threads per workgroup, bins per BatchNorm chunk, chunks per plane, partials per channel, grids
 * of the per-element and the per-bin passes, own kernel launches forward / backward, library calls (1x1 product, Gram, channel
 * sum) forward / backward, 0; then (byte offset, bytes) of the 18 workspace sections [18..53]: the transforms' tables and their complex intermediate, Z (used
 * when nothing is saved), the complex plane the transforms read / write, t, the gate-scaled input (later dt1), pre (later dpre),
 * W'^T dpre (later dt), s, dlogit, the statistics, the BatchNorm partials, W', the three gradient matrices, the fpe / BatchNorm
 * backward partials, the 1x1 / Gram / channel-sum workspaces; the workspace size [60], the saved blob's size [61], the offset of
 * (mu, r) in it [62]; 0.
 * ------------------------------------------------------------------------ */
typedef struct { int B, c, groups, H, W, dtype, training; float eps, momentum; } mi_fourier_unit_shape;
typedef struct {
  const float* bn_w; const float* bn_b; const float* fdc_w; const float* fdc_b; const float* gate_w; const float* gate_b;
  const float* fpe_w; const float* fpe_b;
} mi_fourier_unit_params;
typedef struct {
  float* bn_w; float* bn_b; float* fdc_w; float* fdc_b; float* gate_w; float* gate_b; float* fpe_w; float* fpe_b;
  int accumulate;
} mi_fourier_unit_grads;
size_t mi_fourier_unit_workspace(const mi_fourier_unit_shape* s);
size_t mi_fourier_unit_saved_bytes(const mi_fourier_unit_shape* s);
int mi_fourier_unit_plan(const mi_fourier_unit_shape* s, int64_t* out);
int mi_fourier_unit_fwd(const mi_fourier_unit_shape* s, const mi_fourier_unit_params* p, const void* x, void* out,
                        float* running_mean, float* running_var, void* saved, void* ws, void* stream);
int mi_fourier_unit_bwd(const mi_fourier_unit_shape* s, const mi_fourier_unit_params* p, const void* dout, void* dx,
                        const mi_fourier_unit_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * SFHformer — FFN (SFHformer.py:76-119) and TokenMixer_For_Local (:122-140) over one "segmented depthwise" kernel family
 * (csrc/sfh_ffn.hip): the channel axis is cut into equal segments of s = dim/2 channels, each with its own depthwise stencil
 * (zero padding dil (ks - 1) / 2, weights [s,1,ks,ks], biases [s], fp32) or none.
 *   FFN    x [B,dim,H,W] -> h = conv_init(x) [B,2dim,H,W] (biased 1x1) -> u = (identity | 3x3 | 5x5 | 7x7)(h) over four segments
 *          -> g = gelu_erf(u) -> out = conv_fina(g) [B,dim,H,W] (biased 1x1).
 *          saved: mi_sfh_ffn_saved_bytes(): h and u in the activation dtype, nothing else; saved == NULL in _fwd (inference,
 *          no_grad): nothing is kept and u is never written.  g, dg = W2^T dout and dh live in the workspace; the backward's
 *          stencil kernel multiplies dg by gelu_erf'(u) while staging it, and writes g again for the weight gradient of conv_fina.
 *   local  x [B,dim,H,W] -> cat(3x3 dilation 1 (x[:, :s]), 3x3 dilation 2 (x[:, s:])); no activation; it saves nothing but x.
 * Backward: dx and every parameter gradient (added to when g->accumulate, else overwritten); the stencil gradients are
 * per-workgroup partial rows summed in a fixed order: no atomics, bitwise reproducible.  No allocation, no host synchronisation.
 * Limits: dim even, 2 <= dim <= 256 (an odd dim changes the reference's chunk count: not covered), B, H, W >= 1, B <= 65535,
 * B 2dim H W below 2^31, fp32 or bf16.  Anything else is refused before any launch; the sizing calls return 0.
 * The plan calls (host-only; the launchers and the sizing calls read the same plan) fill out[64]: tile width, tile height,
 * segments, segment width s, the halo of segments 0..3 [4..7], tiles across, tiles down, forward grid x / y / z [10..12],
 * backward splits (workgroups per plane, each walks every splits-th tile), partial rows B splits, partial columns, own kernel
 * launches forward / backward [16, 17], library calls (1x1 product, Gram, channel sum) forward / backward [18, 19], static LDS
 * bytes forward / backward [20, 21], threads per workgroup [22], 0; then (byte offset, bytes) of the workspace sections
 * [24..37]: the 1x1, Gram and channel-sum workspaces, the partial rows, g, dg (inference: h), dh (the local mixer: the partial
 * rows only, the others 0, 0); the workspace size [60], the saved blob's size [61], the offset of u in it [62] (h sits at 0); 0.
 * ------------------------------------------------------------------------ */
typedef struct { int B, dim, H, W, dtype; } mi_sfh_ffn_shape;
typedef struct {
  const float* init_w; const float* init_b;   /* conv_init.0  [2dim,dim], [2dim] */
  const float* c1_w; const float* c1_b;       /* conv1_1.0    [s,1,3,3], [s] */
  const float* c2_w; const float* c2_b;       /* conv1_2.0    [s,1,5,5], [s] */
  const float* c3_w; const float* c3_b;       /* conv1_3.0    [s,1,7,7], [s] */
  const float* fina_w; const float* fina_b;   /* conv_fina.0  [dim,2dim], [dim] */
} mi_sfh_ffn_params;
typedef struct {
  float* init_w; float* init_b; float* c1_w; float* c1_b; float* c2_w; float* c2_b; float* c3_w; float* c3_b; float* fina_w;
  float* fina_b; int accumulate;
} mi_sfh_ffn_grads;
size_t mi_sfh_ffn_workspace(const mi_sfh_ffn_shape* s);
size_t mi_sfh_ffn_saved_bytes(const mi_sfh_ffn_shape* s);
int mi_sfh_ffn_plan(const mi_sfh_ffn_shape* s, int64_t* out);
int mi_sfh_ffn_fwd(const mi_sfh_ffn_shape* s, const mi_sfh_ffn_params* p, const void* x, void* out, void* saved, void* ws,
                   void* stream);
int mi_sfh_ffn_bwd(const mi_sfh_ffn_shape* s, const mi_sfh_ffn_params* p, const void* x, const void* dout, void* dx,
                   const mi_sfh_ffn_grads* g, const void* saved, void* ws, void* stream);
typedef struct { int B, dim, H, W, dtype; } mi_sfh_local_shape;
typedef struct { const float* cd1_w; const float* cd1_b; const float* cd2_w; const float* cd2_b; } mi_sfh_local_params;   /* [s,1,3,3], [s] */
typedef struct { float* cd1_w; float* cd1_b; float* cd2_w; float* cd2_b; int accumulate; } mi_sfh_local_grads;
size_t mi_sfh_local_workspace(const mi_sfh_local_shape* s);
int mi_sfh_local_plan(const mi_sfh_local_shape* s, int64_t* out);
int mi_sfh_local_fwd(const mi_sfh_local_shape* s, const mi_sfh_local_params* p, const void* x, void* out, void* ws, void* stream);
int mi_sfh_local_bwd(const mi_sfh_local_shape* s, const mi_sfh_local_params* p, const void* x, const void* dout, void* dx,
                     const mi_sfh_local_grads* g, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * SFHformer — TokenMixer_For_Gloal (SFHformer.py:183-206) and Mixer (:209-251) (csrc/sfh_mixer.hip), each as one launch sequence
 * over mi_pw_gemm, mi_gram, the channel sum, mi_fourier_unit_*, mi_sfh_local_* and the file's own streaming kernels.
 *   global  b [B,dim,H,W] -> u1 = Wi b + bi [2dim] -> p = gelu_erf(u1) -> f = FourierUnit(2dim, 2dim, groups 4)(p) -> r = f + p
 *           -> u2 = Wf r + bf [dim] -> out = gelu_erf(u2).
 *   mixer   x [B,dim,H,W] -> [a; b] = conv_init(x) as two dense [B,dim,H,W] tensors (one grouped product whose two groups read the
 *           same x and write the halves apart: no slice copy) -> l = local(a),
 *           u2 = global(b) without its last GELU -> g = gelu(cat(l, gelu(u2))) written once into one [B,2dim,H,W] tensor together
 *           with fixed-order partial sums -> per image m = mean g, s = sigmoid(W2 relu(W1 m + b1) + b2) and the folded weight
 *           Wc diag(s_b) [dim,2dim] (one workgroup per image) -> out = (Wc diag(s_b)) g + bc: one mi_pw_gemm with a per-image weight
 *           (never cached: w_bs != 0); s g is never written.
 * running_mean / running_var [4dim] are the FourierUnit's BatchNorm statistics, handled as in mi_fourier_unit_fwd (updated in
 * place when shape.training, on the device; with saved == NULL too).
 * saved (mi_*_saved_bytes(), sections 256-byte aligned, in this order): a, b, l [B,dim,N] (mixer only), u1, r [B,2dim,N], u2
 * [B,dim,N], all in the activation dtype, then the FourierUnit's own blob.  p, f, q, g, m, hidden, s and the folded weights are
 * recomputed or live in the workspace: the backward runs the forward's own tail kernels again over l and u2, so they are the
 * forward's bit for bit.  saved == NULL in _fwd (inference, no_grad): nothing is kept.
 * Backward (mixer): the per-image Gram P_b = dout_b g_b^T (mi_gram, sum_batch = 0); from it dWc = sum_b P_b diag(s_b),
 * ds = sum_m Wc . P_b and the gate's backward (two small kernels: per image, then the sums over the images in order);
 * e = (Wc diag(s_b))^T dout (transposed per-image product); one pass dl = (e + dm/N) gelu'(l), du2 = (e + dm/N) gelu'(q) gelu'(u2);
 * mi_sfh_local_bwd; conv_fina's gradients and dr; mi_fourier_unit_bwd; du1 = (dr + dp) gelu'(u1); the global conv_init's
 * gradients; the mixer's conv_init takes da and db as two K panels (two Grams and two bias sums into the halves of its
 * gradient).  Gradients are added to when g->accumulate, else overwritten.  Bitwise reproducible; no allocation, no host sync.
 * Limits: mixer dim even, 2..128; global dim 1..128; 2 <= H, W <= 512; 1 <= B <= 65535; B 2dim H W below 2^31; fp32 or bf16; and
 * the FourierUnit's own (eps > 0, 0 <= momentum <= 1).  Anything else is refused before any launch; the sizing calls return 0.
 * The plan calls (host-only; launchers and sizing calls read the same plan) fill out[64]: mode (0 global, 1 mixer), B, dim, 2dim,
 * N, pool partials per plane, grid of the flat passes over [B,dim,N] and over [B,2dim,N], grid x of the tail's backward pass,
 * threads per workgroup, own kernel launches forward / backward [10, 11], library calls forward / backward [12, 13], bytes of the
 * backward's planes (e, dl, du2, da, db) inside the scratch section [14], 0; then (byte offset, bytes) of the 13 workspace
 * sections [16..41]: the 1x1, Gram and channel-sum workspaces, the FourierUnit's and the local mixer's workspaces, p (backward:
 * the FourierUnit's input gradient), f (backward: dr, then du1), g, the small fp32 vectors (m, hidden, s, dz2, dz1, dm/N), the
 * folded weights, the per-image Gram, the pool partials, the scratch (forward without a blob: the saved planes without the FourierUnit's blob; backward: e, dl,
 * du2, da, db); then (byte offset, bytes) of the 7 saved sections [44..57]; the workspace size [60], the saved blob's size [61].
 * ------------------------------------------------------------------------ */
typedef struct { int B, dim, H, W, dtype, training; float eps, momentum; } mi_sfh_global_shape;
typedef mi_sfh_global_shape mi_sfh_mixer_shape;
typedef struct {
  const float* init_w; const float* init_b;   /* conv_init.0  [2dim,dim], [2dim] */
  const float* fina_w; const float* fina_b;   /* conv_fina.0  [dim,2dim], [dim] */
  const float* bn_w; const float* bn_b; const float* fdc_w; const float* fdc_b; const float* gate_w; const float* gate_b;
  const float* fpe_w; const float* fpe_b;     /* FFC.*: mi_fourier_unit_params with c = 2dim, groups = 4 */
} mi_sfh_global_params;
typedef struct {
  float* init_w; float* init_b; float* fina_w; float* fina_b; float* bn_w; float* bn_b; float* fdc_w; float* fdc_b; float* gate_w;
  float* gate_b; float* fpe_w; float* fpe_b; int accumulate;
} mi_sfh_global_grads;
typedef struct {
  const float* cd1_w; const float* cd1_b; const float* cd2_w; const float* cd2_b;             /* mixer_local.* */
  const float* init_w; const float* init_b; const float* fina_w; const float* fina_b;         /* mixer_gloal.*, as above */
  const float* bn_w; const float* bn_b; const float* fdc_w; const float* fdc_b; const float* gate_w; const float* gate_b;
  const float* fpe_w; const float* fpe_b;
  const float* cac_w; const float* cac_b;     /* ca_conv.0  [dim,2dim], [dim] */
  const float* ca1_w; const float* ca1_b;     /* ca.1       [dim,2dim], [dim] */
  const float* ca2_w; const float* ca2_b;     /* ca.3       [2dim,dim], [2dim] */
  const float* conv_w; const float* conv_b;   /* conv_init.0 [2dim,dim], [2dim] */
} mi_sfh_mixer_params;
typedef struct {
  float* cd1_w; float* cd1_b; float* cd2_w; float* cd2_b; float* init_w; float* init_b; float* fina_w; float* fina_b; float* bn_w;
  float* bn_b; float* fdc_w; float* fdc_b; float* gate_w; float* gate_b; float* fpe_w; float* fpe_b; float* cac_w; float* cac_b;
  float* ca1_w; float* ca1_b; float* ca2_w; float* ca2_b; float* conv_w; float* conv_b; int accumulate;
} mi_sfh_mixer_grads;
size_t mi_sfh_global_workspace(const mi_sfh_global_shape* s);
size_t mi_sfh_global_saved_bytes(const mi_sfh_global_shape* s);
int mi_sfh_global_plan(const mi_sfh_global_shape* s, int64_t* out);
int mi_sfh_global_fwd(const mi_sfh_global_shape* s, const mi_sfh_global_params* p, const void* x, void* out, float* running_mean,
                      float* running_var, void* saved, void* ws, void* stream);
int mi_sfh_global_bwd(const mi_sfh_global_shape* s, const mi_sfh_global_params* p, const void* x, const void* dout, void* dx,
                      const mi_sfh_global_grads* g, const void* saved, void* ws, void* stream);
size_t mi_sfh_mixer_workspace(const mi_sfh_mixer_shape* s);
size_t mi_sfh_mixer_saved_bytes(const mi_sfh_mixer_shape* s);
int mi_sfh_mixer_plan(const mi_sfh_mixer_shape* s, int64_t* out);
int mi_sfh_mixer_fwd(const mi_sfh_mixer_shape* s, const mi_sfh_mixer_params* p, const void* x, void* out, float* running_mean,
                     float* running_var, void* saved, void* ws, void* stream);
int mi_sfh_mixer_bwd(const mi_sfh_mixer_shape* s, const mi_sfh_mixer_params* p, const void* x, const void* dout, void* dx,
                     const mi_sfh_mixer_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * SFHformer — the Block's BatchNorm2d and scaled residual (SFHformer.py:254-282; csrc/bn2d.hip).  x, y, f, out and the cotangents
 * [B,C,H,W] in `dtype`, N = H W, n = B N; w, b, scale, running_mean, running_var, stat and every parameter gradient fp32; fp32
 * arithmetic between load and store, one rounding to `dtype` at the store.
 *   BatchNorm2d, training:  mu[c] = mean of x over the n values of channel c, var[c] = their biased variance,
 *        r[c] = 1 / sqrt(var[c] + eps),  y = (x - mu[c]) (w[c] r[c]) + b[c], and in the same launch sequence, in place, on the device
 *        running_mean <- (1 - momentum) running_mean + momentum mu,
 *        running_var  <- (1 - momentum) running_var  + momentum var n / (n - 1)       (num_batches_tracked is the caller's).
 *        A plane is cut into chunks of 4096 elements; one workgroup holds one chunk in registers and writes its (mean, sum of
 *        squared deviations from that mean), so x is read once and two large sums are never differenced; one thread per channel
 *        merges the channel's B nchunk pairs, image by image and chunk by chunk (Chan's update).  The pairs are laid out
 *        [B][C][nchunk][2].
 *   BatchNorm2d, eval:  mu = running_mean, r = 1 / sqrt(running_var + eps); nothing is updated; ONE launch.
 *   stat [2C] = (mu[C], r[C]) is what the backward needs beside x; stat == NULL in _fwd (inference, no_grad): it lives in the
 *        workspace (training mode still updates the running statistics).
 *   part_in != NULL (training): the pairs are taken from there, in the layout above, and the statistics pass is skipped; what
 *        mi_scale_res_fwd(..., part_out) writes for the same shape are those pairs, bit for bit.  Ignored in eval mode.
 *   backward:  xhat = (x - mu) r;  db (+)= sum dy;  dw (+)= sum dy xhat  (`accumulate` adds, else overwrites; per-chunk partial
 *        rows summed in the order above);  training: dx = w r ((dy - sum dy / n) - xhat (sum dy xhat) / n);  eval: dx = w r dy.
 *        dres != NULL: dx + dres is written instead, added in fp32 and rounded once.  `stat` is the forward's.
 *   scaled residual:  out = f scale[c] + x.   part_out != NULL: also the BatchNorm pairs of out AS STORED (after the rounding to
 *        `dtype`), part_out [B][C][nchunk][2] floats (bytes: plan [62]).
 *        backward, one pass over f and dout:  df = dout scale[c];  dscale[c] (+)= sum f dout.  The gradient towards x is dout
 *        itself: nothing is written for it.  The shape's training, eps and momentum are not read.
 * Limits: 1 <= C <= 4096; B, H, W >= 1; B C H W below 2^31; fp32 or bf16; BatchNorm: eps > 0, 0 <= momentum <= 1, and training with
 * n = 1 is refused (no variance).  Anything else is refused before any launch (the message: mi_last_error); the sizing calls
 * return 0.  16-byte accesses where N is a multiple of 16 / sizeof(dtype) and the pointers are 16-byte aligned, element by element
 * otherwise, over the same assignment of elements to threads: the results do not depend on which form ran.  Bitwise reproducible
 * (no atomics, every sum in a fixed order).  No allocation, no host synchronisation.
 * The plan calls (host-only; the launchers and the sizing calls read the same plan) fill out[64]: B, C, N, dtype, training, threads
 * per workgroup, chunk size, chunks per plane, partials per channel (B nchunk), elements per access the shape allows (4 / 8, or 1),
 * chunks of work B C nchunk, grid of the per-chunk launches (capped at 2^20, the rest by a grid stride), grid of the per-channel
 * finish launches, launches forward / forward with part_in / backward [13..15]; then (byte offset, bytes) of the workspace
 * sections [16..21]: the partial rows (BatchNorm: pairs, forward and backward; scaled residual: the sums of f dout), stat (used
 * when none is given), the backward's two means (scaled residual: 0, 0); the workspace size [60], the bytes of stat [61], the
 * bytes of the pairs part_in / part_out hold [62]; 0.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, H, W, dtype, training; float eps, momentum; } mi_bn2d_shape;
typedef mi_bn2d_shape mi_scale_res_shape;
size_t mi_bn2d_workspace(const mi_bn2d_shape* s);
int mi_bn2d_plan(const mi_bn2d_shape* s, int64_t* out);
int mi_bn2d_fwd(const mi_bn2d_shape* s, const float* w, const float* b, const void* x, void* y, float* running_mean,
                float* running_var, float* stat, const float* part_in, void* ws, void* stream);
int mi_bn2d_bwd(const mi_bn2d_shape* s, const float* w, const void* x, const void* dy, const void* dres, void* dx, float* dw,
                float* db, int accumulate, const float* stat, void* ws, void* stream);
size_t mi_scale_res_workspace(const mi_scale_res_shape* s);
int mi_scale_res_plan(const mi_scale_res_shape* s, int64_t* out);
int mi_scale_res_fwd(const mi_scale_res_shape* s, const float* scale, const void* f, const void* x, void* out, float* part_out,
                     void* stream);
int mi_scale_res_bwd(const mi_scale_res_shape* s, const float* scale, const void* f, const void* dout, void* df, float* dscale,
                     int accumulate, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * SFHformer — Block (SFHformer.py:254-282; csrc/sfh_block.hip) as one launch sequence forward and one backward over the entry
 * points above; the file has no kernel and no arithmetic of its own.
 *   forward   y1 = mi_bn2d_fwd(x; part_in)        m = mi_sfh_mixer_fwd(y1)     x1 = mi_scale_res_fwd(m, x, beta; part_out = p1)
 *             y2 = mi_bn2d_fwd(x1; part_in = p1)  f = mi_sfh_ffn_fwd(y2)       out = mi_scale_res_fwd(f, x1, gamma; part_out)
 *   backward  df, dgamma = mi_scale_res_bwd(f, dout)     dy2 = mi_sfh_ffn_bwd(y2, df)       dx1 = mi_bn2d_bwd(x1, dy2; dres = dout)
 *             dm, dbeta  = mi_scale_res_bwd(m, dx1)      dy1 = mi_sfh_mixer_bwd(y1, dm)     dx  = mi_bn2d_bwd(x, dy1; dres = dx1)
 * The results are those of the six calls made one by one, bit for bit.  One eps / momentum pair serves norm1, norm2 and the
 * Mixer's FFC.bn.  part_in: the (mean, M2) pairs of x (mi_bn2d_fwd's part_in) or NULL; part_out: where the pairs of out go, or
 * NULL (a following Block's part_in); p1 lives in the workspace.  Eval mode (shape.training == 0) reads and writes no pairs: both
 * are ignored.  stats: the running statistics of norm1, norm2 [dim] and of the Mixer's FFC.bn [4 dim], updated in place in
 * training mode.
 * saved (mi_sfh_block_saved_bytes(), sections 256-byte aligned, in this order): y1, m, x1, y2, f [B,dim,N] in the activation
 * dtype, stat1, stat2 [2 dim] fp32, the Mixer's blob, the FFN's blob.  saved == NULL in _fwd (inference, no_grad): nothing is
 * kept, the five planes live in the workspace and the Mixer and the FFN run with their own saved == NULL.
 * Gradients are added to when g->accumulate, else overwritten (the `accumulate` fields of the embedded structs are not read).
 * Limits, the intersection of the parts': dim even, 2..128; 2 <= H, W <= 512; 1 <= B <= 65535; fp32 or bf16; eps > 0,
 * 0 <= momentum <= 1; the parts' size limits (B 4dim H W below 2^31 among them).  Anything else is refused before any launch; the
 * sizing calls return 0.  Bitwise reproducible; no allocation, no host synchronisation.
 * mi_sfh_block_plan (host-only; launchers and sizing calls read the same plan) fills out[64]: B, dim, N, chunks per plane of the
 * BatchNorm kernels, library calls forward / forward with part_in / backward [4..6], kernel launches of those calls' own
 * forward / forward with part_in / backward [7..9] (summed from the parts' plans), library calls the Mixer and the FFN make in
 * turn forward / backward [10, 11]; then (byte offset, bytes) of the 6 workspace sections [16..27]: the region the parts'
 * workspaces share (the calls are sequential on one stream), the pairs p1 (eval: 0 bytes), the backward's three planes (df then
 * dm; dy2 then dy1; dx1), the scratch of a forward without a blob; then of the 9 saved sections [32..49]; the workspace size
 * [60], the saved blob's size [61], the bytes part_in / part_out hold [62] (mi_bn2d_plan's).
 * ------------------------------------------------------------------------ */
typedef mi_sfh_mixer_shape mi_sfh_block_shape;
typedef struct {
  const float* bn1_w; const float* bn1_b;     /* norm1 [dim] */
  mi_sfh_mixer_params mixer;                  /* mixer.* */
  const float* beta;                          /* [1,dim,1,1] */
  const float* bn2_w; const float* bn2_b;     /* norm2 [dim] */
  mi_sfh_ffn_params ffn;                      /* ffn.* */
  const float* gamma;                         /* [1,dim,1,1] */
} mi_sfh_block_params;
typedef struct {
  float* bn1_w; float* bn1_b; mi_sfh_mixer_grads mixer; float* beta; float* bn2_w; float* bn2_b; mi_sfh_ffn_grads ffn; float* gamma;
  int accumulate;
} mi_sfh_block_grads;
typedef struct { float* mean1; float* var1; float* mean2; float* var2; float* mean_fu; float* var_fu; } mi_sfh_block_stats;
size_t mi_sfh_block_workspace(const mi_sfh_block_shape* s);
size_t mi_sfh_block_saved_bytes(const mi_sfh_block_shape* s);
int mi_sfh_block_plan(const mi_sfh_block_shape* s, int64_t* out);
int mi_sfh_block_fwd(const mi_sfh_block_shape* s, const mi_sfh_block_params* p, const void* x, void* out,
                     const mi_sfh_block_stats* stats, const float* part_in, float* part_out, void* saved, void* ws, void* stream);
int mi_sfh_block_bwd(const mi_sfh_block_shape* s, const mi_sfh_block_params* p, const void* x, const void* dout, void* dx,
                     const mi_sfh_block_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * DarkIR — the encoder block (DarkIR-main/archs/arch_model.py:141-204 EBlock) and its tail (csrc/darkir.hip).
 *
 * fregate: the block's last line, y + gamma (y f), as one streaming pass.  y, f, out [B,C,N] in `dtype`, gamma [C] fp32, fp32
 * arithmetic:   out = y (1 + gamma[c] f).
 *   bwd (one pass over dout, y, f):  df = (dout gamma[c]) y;  dyr = dout (1 + gamma[c] f);  dgamma[c] (+)= sum_{b,p} (dout y) f
 *   (per-workgroup partial rows summed in a fixed order: no atomics, bitwise reproducible; accumulate != 0 adds to dgamma).
 * 16-byte vector access over the aligned interior of every plane, scalar head and tail; any N >= 1, any alignment the dtype has
 * (pointers that disagree modulo 16 bytes take the scalar form).  B, C <= 65535.  ws: mi_fregate_bwd_workspace() bytes.
 *
 * EBlock.forward / backward as one unit:
 *   x0 = LayerNorm2d(inp; norm1, eps 1e-6);  xe = extra_conv(x0) when `extra` (plain depthwise 3x3, w [c, 9]), else x0;
 *   x1 = conv1(xe) [2c];  g = dilgate(x1);  s[b] = sca_w . mean_hw(g[b]) + sca_b;  y = inp + beta (conv3(s g));
 *   f = FreMLP(LayerNorm2d(y; norm2)) (nc = c, expand = 2: fre_w1 [2c, c], fre_w2 [c, 2c]);  out = fregate(y, f, gamma).
 * The pieces are mi_ln_fwd_eps, mi_dwconv_*, the split-weight 1x1 products and the per-image fold of DBlock, mi_dilgate_*,
 * mi_fremlp_* and mi_fregate_*.  Parameters fp32 in the reference's layout, every bias required; extra_w / extra_b are read only
 * when `extra`.  saved == NULL: inference, nothing is kept.  Kept for the backward: x0, xe (with `extra`), x1, g, y, f, the
 * LayerNorm statistics, pool, s, the folded conv3 matrices and the FreMLP blob; LayerNorm2d(y) is not (FreMLP's backward reads
 * its blob only).
 * Limits: 1 <= C <= 256, 2 <= H, W <= 512, 1..4 dilations of 1..16, fp32 or bf16, 2 C H W < 2^31 and FreMLP's own size
 * conditions; anything else is refused before any launch and the sizing calls return 0.
 * mi_eblock_plan (host-only; the sizing calls and the launchers read the same layout) fills out[16]: bytes of x0, xe (0 without
 * `extra`), x1, g, y, f, of the four LayerNorm statistics, of the small tensors (pool, s, the conv3 folds), of the FreMLP blob;
 * saved bytes; workspace bytes; calls of the forward's / the backward's launch sequence (a library entry point counts as one,
 * FreMLP as its own launches and library calls); workgroups per plane of the fregate backward; 0; 0.
 * ------------------------------------------------------------------------ */
typedef struct { int B, C, H, W, dtype, n_dil; int dil[4]; int extra; } mi_eblock_shape;
typedef struct {
  const float* norm1_w; const float* norm1_b; const float* extra_w; const float* extra_b; const float* conv1_w; const float* conv1_b;
  const float* br_w[4]; const float* br_b[4];
  const float* sca_w; const float* sca_b; const float* conv3_w; const float* conv3_b; const float* beta;
  const float* norm2_w; const float* norm2_b; const float* fre_w1; const float* fre_b1; const float* fre_w2; const float* fre_b2;
  const float* gamma;
} mi_eblock_params;
typedef struct {
  float* norm1_w; float* norm1_b; float* extra_w; float* extra_b; float* conv1_w; float* conv1_b;
  float* br_w[4]; float* br_b[4];
  float* sca_w; float* sca_b; float* conv3_w; float* conv3_b; float* beta;
  float* norm2_w; float* norm2_b; float* fre_w1; float* fre_b1; float* fre_w2; float* fre_b2;
  float* gamma;
  int accumulate;
} mi_eblock_grads;
int mi_fregate_fwd(const void* y, const void* f, const float* gamma, void* out, int B, int C, int64_t N, int dtype, void* stream);
size_t mi_fregate_bwd_workspace(int B, int C, int64_t N);
int mi_fregate_bwd(const void* dout, const void* y, const void* f, const float* gamma, void* df, void* dyr, float* dgamma, int B,
                   int C, int64_t N, int accumulate, int dtype, void* ws, void* stream);
size_t mi_eblock_saved_bytes(const mi_eblock_shape* s);
size_t mi_eblock_workspace(const mi_eblock_shape* s);
int mi_eblock_plan(const mi_eblock_shape* s, int64_t* out);
int mi_eblock_fwd(const mi_eblock_shape* s, const mi_eblock_params* p, const void* inp, void* out, void* saved, void* ws,
                  void* stream);
int mi_eblock_bwd(const mi_eblock_shape* s, const mi_eblock_params* p, const void* inp, const void* dout, void* dinp,
                  const mi_eblock_grads* g, const void* saved, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * The other pixel-space loss terms of the reference's training steps (csrc/losses.hip), each with d loss / d pred from the same
 * call.  Conventions of mi_fft_l1_loss: fp32 arithmetic on inputs widened on load; dpred written in `dtype`, rounded once, NULL
 * skips every gradient stage; loss is device fp32 and overwritten; ws holds the matching *_workspace() bytes; no atomics,
 * fixed-order sums (bitwise reproducible); no allocation, no host synchronisation; every refusal returns before any launch.
 *
 * mi_ssim_loss   SSIMloss / SSIM (MoCE-IR-main/src/utils/loss_utils.py:35-55), i.e. pytorch_msssim.ssim with its defaults,
 *                restated (that library is not a dependency: this definition is the contract, unpinned like mi_psnr_ssim):
 *                window g[i] = exp(-(i-5)^2 / (2 1.5^2)), i = 0..10, sum 1, separable, per channel, VALID correlation (the map
 *                is (H-10) x (W-10));  C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;  mu1 = g*x, mu2 = g*y,
 *                s1 = g*x^2 - mu1^2, s2 = g*y^2 - mu2^2, s12 = g*xy - mu1 mu2,
 *                S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  m = mean of S over B C (H-10)(W-10).
 *                loss[0] = loss_weight (1 - m), loss[1] = m (loss holds TWO floats);  dpred = d loss[0] / d pred.
 *                H, W >= 11, data_range > 0.  Kernels work on MI_SSIM_TILE x MI_SSIM_TILE tiles of the map / the image.
 * mi_edge_loss   EdgeLoss (loss_utils.py:155-190) for any C >= 1, H, W >= 2:  e = L(pred - target),  L(c) = c - G(Z),
 *                G the 5x5 blur [.05 .25 .4 .25 .05]^T [.05 .25 .4 .25 .05] over the replicate-padded plane, Z = 4 G(c) at
 *                even (row, col) and 0 elsewhere.  criterion 0 ('l2'): loss = loss_weight mean(e^2), dpred = loss_weight
 *                (2/N) L^T e;  criterion 1 ('l1'): loss = loss_weight mean|e|, dpred = loss_weight (1/N) L^T sign(e), sign(0) = 0.
 * mi_focal_l1_loss  FocalL1Loss (loss_utils.py:100-136), flat over n elements:  a = |pred - target| / alpha,
 *                loss = scale mean(log1p(a + epsilon)^gamma a),  dpred its gradient, sign(0) = 0 (exactly 0 at a tie).
 *                alpha > 0, gamma >= 0, epsilon >= 0.
 * ------------------------------------------------------------------------ */
#define MI_SSIM_TILE 32
size_t mi_ssim_loss_workspace(int B, int C, int H, int W);
int mi_ssim_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                 float loss_weight, float data_range, int dtype, void* ws, void* stream);
size_t mi_edge_loss_workspace(int B, int C, int H, int W);
int mi_edge_loss(const void* pred, const void* target, void* dpred, float* loss, int B, int C, int H, int W,
                 float loss_weight, int criterion, int dtype, void* ws, void* stream);
size_t mi_focal_l1_workspace(int64_t n);
int mi_focal_l1_loss(const void* pred, const void* target, void* dpred, float* loss, int64_t n, float gamma, float epsilon,
                     float alpha, float scale, int dtype, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * Optional per-kernel profiler (measurement aid for bench.py's roofline object; nothing in the
 * reference corresponds to it).  When enabled every kernel launch is bracketed by two HIP events
 * recorded on the stream it is launched on, and its algorithmic HBM bytes / flops are booked.
 * mi_prof_collect synchronises, fills per-kernel-id totals (arrays of mi_prof_kernel_count()
 * entries: milliseconds, algorithmic bytes, flops, launches).  mi_prof_enable(1|0) clears records.
 * Not for use inside HIP-graph capture.
 * ------------------------------------------------------------------------ */
int mi_prof_enable(int on);
int mi_prof_kernel_count(void);
const char* mi_prof_kernel_name(int kid);
int mi_prof_collect(double* ms, double* bytes, double* flops, int64_t* launches, int n);

#ifdef __cplusplus
}
#endif
#endif /* MI_RESTORE_H */
