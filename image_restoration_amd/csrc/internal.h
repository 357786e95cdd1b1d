// Internal launchers shared between translation units (not part of the C-ABI).
#pragma once
#include <initializer_list>

#include "common.h"

namespace mi {
// kernel-side view of mi_pw_desc (strides in elements)
struct PwK {
  const void* x1; int64_t x1_bs, x1_gs; int k1;
  const void* x2; int64_t x2_bs, x2_gs; int k2;
  const float* w; int64_t w_bs, w_gs, w_sm, w_sk;
  const float* bias; int64_t bias_gs;
  const void* r; int64_t r_bs, r_gs;
  void* y; int64_t y_bs, y_gs;
  int m; int64_t n; int groups; int vec_ok;
  void* y2; int64_t y2_bs, y2_gs; int y_split;   // rows >= y_split go to y2 (wave-owned forms, no residual); 0 = one output
};
// What one mi_pw_gemm call runs: filled by pw_plan (pw_gemm.hip), the ONE place that decides it; the launchers launch what it
// says, the mi_pw_gemm_*_ok predicates and mi_pw_gemm_workspace read it, mi_pw_plan reports it.
enum PwFamily { PW_CHUNKED = 0, PW_RESIDENT, PW_DMA, PW_XRES, PW_STREAM, PW_XWIDE, PW_LDS };
enum PwWeights { PW_W_PACK = 0, PW_W_B16, PW_W_F32 };   // own packed image / the producer's bf16 copy / straight from fp32
struct PwPlan {
  int family;                                    // PwFamily
  int tm, m_tiles, k_chunks;                     // the instance: rows per tile, tiles over M, K chunks (32 deep; PW_LDS: 64)
  bool f8, ln;                                   // ... and its fp8 / LayerNorm-on-load template choices
  bool vec_ok;                                   // 16-byte rows: every pointer and stride allows vector access
  int slices, per_batch, per_group, chunk_elems; // the pw_pack image: [slice][m-tile][k-chunk][chunk_elems]
  int64_t slice_elems;
  size_t bytes;                                  // ... its size with the zero block (sized for every family: mi_pw_gemm_workspace)
  size_t lds_image;                              // the LDS-tiled kernel's image, wherever dtype and depth could reach that kernel
  dim3 grid, block; size_t lds;                  // the launch
  int tpw, tpb, n_slabs, slabs_per, xcd_map;     // pixel tiles per wave (wave forms) / per workgroup (resident); X-wide M slabs
  int weights;                                   // PwWeights
  bool cacheable;                                // may use the packed-weight cache (static weights, own pack)
  size_t ws_bytes() const { return family == PW_LDS ? align_up(lds_image, 256) : bytes; }   // what this call's workspace holds
};
// What one mi_gram call runs: filled by gram_plan (gram.hip), the ONE place that decides it; mi_gram launches and finishes as it
// says, mi_gram_workspace sizes from it, mi_gram_plan reports it.
enum GramFamily { GRAM_LDS = 0, GRAM_STREAM };   // LDS-staged tiles (either dtype) / register-streaming (bf16, 16-byte rows)
enum GramFinish { GRAM_DIRECT = 0, GRAM_REDUCE_FEW4, GRAM_REDUCE_FEW16, GRAM_REDUCE };   // straight into the output / which kernel sums the partials
struct GramPlan {
  int family;                                    // GramFamily
  int fa, fb; bool ss;                           // the instance: fragments per tile side (32 rows each; streaming: 16), sumsq rows (their row sum follows)
  int unit, units, per_split;                    // contraction unit in pixels (32 / 64), units in total (folded: of all images), per workgroup
  int splits, tiles_a, tiles_b, Z, fold;         // fold > 0: the batch is chained along the pixel axis, `fold` units per image
  bool vec_ok;                                   // 16-byte rows: every pointer and stride allows vector access
  dim3 grid, block;                              // the launch
  size_t part_bytes, ss_bytes;                   // partial tiles [splits][Z][ma][mb]; sumsq rows [splits][Z][ma+mb] (sized whether asked for or not)
  int finish;                                    // GramFinish
  bool deferrable;                               // the partials may go to the deferred arena instead (summed at its flush)
  int images, total, zo;                         // the reduce: images a partial keeps apart, partials per output element, output slices
  size_t ws_bytes() const { return part_bytes + ss_bytes; }   // the workspace of this plan, sumsq rows reserved
};
// Launch with dynamic LDS: above 64 KiB the kernel's limit has to be raised first.
template <typename... P, typename... A>
static inline int launch_dyn_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds > 64 * 1024) MI_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int launch_attn_fold(const float* graw, const float* ss, const float* temperature, const float* wo, float* P, float* A,
                     float* nrm, float* M, int B, int C, int heads, hipStream_t st, void* Mb = nullptr, void* Mtb = nullptr);
int launch_attn_bwd_small(const float* dM, const float* A, const float* P, const float* nrm, const float* temperature,
                          const float* wo, float* dwo_part, float* dtemp_part, float* wd, float* scratch,
                          int B, int C, int heads, hipStream_t st, void* wdb = nullptr);
size_t attn_bwd_scratch_floats(int B, int C, int heads);
// ---- top-k sparse attention, the c x c side (tksa.hip): drop-in for launch_attn_fold / launch_attn_bwd_small ----
struct TopkArgs { const float* w[4]; int k[4]; };   // attn1..attn4 (device scalars) and the four top-k sizes
int tksa_check(int C, int heads, const int* k);
int launch_tksa_fold(const float* graw, const float* ss, const float* temperature, const TopkArgs& tk, const float* wo, float* P,
                     float* S, float* A, float* nrm, float* M, float* scores, int B, int C, int heads, hipStream_t st, void* Mb,
                     void* Mtb);
int launch_tksa_bwd(const float* dM, const float* A, const float* S, const float* P, const float* nrm, const float* temperature,
                    const TopkArgs& tk, const float* wo, float* dwo_part, float* dtemp_part, float* dattn_part, float* wd, int B,
                    int C, int heads, hipStream_t st, void* wdb);
// ---- mixed-scale FFN stencils (msfn.hip) ----
int msfn_splits(int H, int W);
size_t msfn_part_floats(int B, int hd, int H, int W);
int launch_msfn_s1_fwd(const void* h0, const float* w3, const float* b3, const float* w5, const float* b5, void* a, void* b, int B,
                       int hd, int H, int W, int dtype, hipStream_t st);
int launch_msfn_s2_fwd(const void* a, const void* b, const float* g3w, const float* g3b, const float* g5w, const float* g5b, void* y,
                       int B, int hd, int H, int W, int dtype, hipStream_t st);
int launch_msfn_s2_bwd(const void* dY, const void* y, const void* a, const void* b, const float* g3w, const float* g5w, void* dza,
                       void* dzb, float* g_g3w, float* g_g3b, float* g_g5w, float* g_g5b, int accumulate, float* part, int B, int hd,
                       int H, int W, int dtype, hipStream_t st);
int launch_msfn_s1_bwd(const void* dza, const void* dzb, const void* h0, const float* w3, const float* w5, void* dh0, float* g_w3,
                       float* g_b3, float* g_w5, float* g_b5, int accumulate, float* part, int B, int hd, int H, int W, int dtype,
                       hipStream_t st);
size_t chan_sum_workspace(int C, int64_t N);
int launch_chan_sum(const void* x, float* out, int B, int C, int64_t N, int dtype, int accumulate, void* ws, hipStream_t st);
#if defined(__HIPCC__)
// Sums NV per-thread values over a workgroup of 256 threads (wave DPP sums, then the 4 waves in order: a fixed order, bitwise
// reproducible); thread n < NV gets total n.  red: 4 * NV floats of LDS.  Used by the stencil backwards (msfn.hip, sfh_ffn.hip).
template <int NV>
__device__ __forceinline__ float block_sum4(const float (&v)[NV], float* red) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    const float s = wave_sum(v[n]);
    if (lane == 0) red[wv * NV + n] = s;
  }
  __syncthreads();
  const int n = threadIdx.x;
  return n < NV ? (red[n] + red[NV + n]) + (red[2 * NV + n] + red[3 * NV + n]) : 0.f;
}
#endif

// ---- depthwise convolution (dwconv.hip: LDS-tiled k x k; dwstream.hip: register-streaming 3x3) ----
enum { IN_PLAIN = 0, IN_GATE_BWD = 1 };
struct DwArgs {
  const void* in;     // plain: x / dy  [B,Cc,H,W]
  const void* gy;     // gate-bwd: conv outputs y [B,2h,H,W] (in = dg [B,h,H,W])
  const float* w;     // [Cc, KS*KS]
  const float* bias;  // [Cc] or null
  void* out;          // [B,Cc,H,W] (may be null in gate fwd)
  void* gate;         // gate fwd: g [B,h,H,W]
  int Cc, H, W, hidden, tiles_x;
};
// Streaming 3x3 path: usable when the row is 16..256 pixels, a power of two, and every plane base is 16-byte aligned.
bool dws_eligible(int H, int W, int ks);
int dws_partial_rows(int B, int H, int W, int64_t planes);  // rows of weight-gradient partials the backward kernels write
void dws_plan(int H, int W, int64_t planes, int* band, int* nb, int* lpr, int* uni);  // the launch plan (mi_dwconv_plan)
int dws_fwd(const DwArgs& a, int B, bool gate, bool flip, int dtype, hipStream_t st);
int dws_bwd(const DwArgs& dya, const void* xin, float* part, int B, bool want_dx, int* rows_out, int dtype, hipStream_t st);
int dws_gate_bwd(const DwArgs& a, const void* xin, float* part, int B, bool want_dw, int* rows_out, int dtype,
                 hipStream_t st);
// same, with the conv outputs recomputed from the conv input: a.in = dg, a.gy = conv input x, a.bias = conv bias
int dws_gate_bwd_recompute(const DwArgs& a, float* part, int B, bool want_dw, int* rows_out, int dtype, hipStream_t st);
// ---- backward tail of a half-block (bwd_tail.hip): dW, W^T dY, LayerNorm backward and the residual add in one launch ----
// What one mi_bwd_tail call runs: filled by bwd_tail_plan (bwd_tail.hip), the ONE place that decides it; launch_bwd_tail launches
// what it says, the three predicates below answer from it, mi_bwd_tail_plan reports it.  Not covered: every field 0.
struct BtPlan {
  bool covered, pays;                            // the kernel takes the call / and beats the unfused chain (MI_BT_WIDE)
  int C, NW, MPW, rows, mpad;                    // the instance: waves, 16-row fragments per wave, rows per wave, rows in all
  int grid, launch;                              // workgroups the partials are sized for / launched (min(tiles, grid))
  int64_t tiles_per_image, tiles;                // 64-pixel tiles
  int passes, active;                            // trips of the persistent loop (ceil(tiles / launch)); waves that hold rows
  size_t lds, ws_bytes;                          // dynamic LDS; the workspace (partials [grid][M][C + 1] and the row sum's scratch)
};
BtPlan bwd_tail_plan(int M, int C, int B, int64_t N, int dtype);
bool bwd_tail_ok(int M, int C, int64_t N, int dtype);
bool bwd_tail_pays(int M, int C);   // covered AND faster than the unfused chain (the module entry points use the tail only then)
size_t bwd_tail_workspace(int M, int C);
int launch_bwd_tail(const void* dy, int M, const void* x, int C, const void* dres, const float* mean, const float* rstd,
                    const float* w, const float* gamma, const float* beta, void* dx, float* dw, float* dgamma, float* dbeta,
                    int B, int64_t N, int accumulate, void* ws, hipStream_t st);
// ---- LDS-tiled 1x1 GEMM for deep K (pw_lds.hip): the PW_LDS family of pw_plan, which decides where it runs ----
#define MI_HIDDEN __attribute__((visibility("hidden")))   // (internal: not in the library's dynamic symbol list)
MI_HIDDEN int pw_lds_tm(int M);                 // its tile height (256 / 128 rows)
MI_HIDDEN size_t pw_lds_lds_bytes(int tm);      // dynamic LDS of the instance with that tile height
MI_HIDDEN int pw_lds_launch(const mi_pw_desc* d, const PwPlan& pl, void* ws, hipStream_t st);   // packs its image into ws, then launches
// ---- the real 2-D transforms (dft2.hip) have a header of their own, dft2.h: geometry, tables, stages and the four directions ----
// ---- fused GDFN forward, training form (fused_gdfn.hip): also writes h0 [B][2h][H][W] and g [B][h][H][W] ----
int fused_gdfn_fwd_save(const mi_gdfn_fused_shape* s, const void* pack, const void* y, void* out, float* mean, float* rstd,
                        void* h0, void* g, hipStream_t st);
// What one fused GDFN forward runs: filled by fg_plan (fused_gdfn.hip), the ONE place that decides it and that reads MI_FG_CFG /
// MI_FG_NOXCD; the three launchers launch what it says, mi_gdfn_fused_ok / _pack_bytes / _pack / _fwd_train_ok answer from it,
// mi_gdfn_fused_plan reports it.  An entry with no instance under the current switches: covered = false and every field 0.
enum FgEntry { FG_INFER = 0, FG_TRAIN, FG_F8 };   // mi_gdfn_fused_fwd / mi_gdfn_fused_fwd_train / mi_gdfn_fused_fwd_f8
enum FgFamily { FG_TILE = 0, FG_FOURTH };         // fg_fwd_kernel (conv on the VALU) / fg4_fwd_kernel (conv on the matrix cores, persistent)
struct FgPlan {
  bool covered;
  int family;                                    // FgFamily
  int C, th, tw, pc, nw; bool save, f8;          // the instance: tile rows / columns, gate pairs per chunk, waves, SAVE / F8 template choices
  int nch, ngr;                                  // chunks of pc pairs (tile family) / groups of two 16-pair chunks, even (fourth form)
  int tiles_x, tiles_y, S;                       // tiles of an image; workgroups per image (tile family: one per tile; fourth form: persistent ranges)
  int64_t grid; int block; size_t lds;           // B * S workgroups, threads, dynamic LDS
  bool xcd_pairs;                                // tile relabelling that puts vertical neighbours on one XCD (TW = 32, B * tiles % 16 == 0)
  size_t pack_bytes; int pack_pc;                // the blob (tile sections sized for either chunk width, then the fourth form's), and the
};                                               // chunk width its tile sections are built for / read with under the current switches
MI_HIDDEN FgPlan fg_plan(const mi_gdfn_fused_shape* s, int entry);
// What one fused MDTA forward (pass A) runs: filled by fm_plan (fused_mdta.hip), the ONE place that decides it and that reads
// MI_FM_CFG; mi_mdta_fused_ok / _pays / _pack_bytes / _workspace / _fwd answer from it, mi_mdta_fused_plan reports it.
enum FmForm { FM_ROUND3 = 0, FM_FOURTH };         // fm_fwd_kernel (conv on the VALU) / fm4_fwd_kernel (conv on the matrix cores)
struct FmPlan {
  bool covered, pays;                            // the kernel takes the shape / and fills the chip (B * S >= 192 of the 256 CUs)
  int kind, form;                                // 1: C 48 one head, 2: C 96 two heads, 3: C 96 one head; FmForm
  int C, heads, th, nw;
  int tiles_x, tiles_y, S;                       // 8 x 32 tiles of an image; persistent workgroups per image (each a contiguous tile range)
  int64_t grid; int block; size_t lds;
  int part_mult;                                 // Gram partials a workgroup writes (fourth form: one per wave)
  size_t part_bytes, ws_bytes, pack_bytes;       // the partials' arena (sized for 8 per workgroup in either form), the workspace, the blob
};
MI_HIDDEN FmPlan fm_plan(const mi_mdta_shape* s);

// ---- host vocabulary of the module launch sequences (modules.hip, mefc.hip, fused_mdta.hip) ----
static inline size_t fbytes(size_t n) { return align_up(n * sizeof(float), 256); }
static inline size_t tbytes(size_t n, int dt) { return align_up(n * dtype_size(dt), 256); }
static inline size_t max_of(std::initializer_list<size_t> v) {
  size_t m = 0;
  for (size_t x : v) m = x > m ? x : m;
  return m;
}
// A module's workspace (or saved blob) as N sections, each on a 256-byte boundary: the plan fills it, the launchers take their
// pointers from it, the plan report lists it.  It starts zeroed with the plan that holds it.
template <int N> struct Sections {
  size_t off[N], bytes[N], total;
  void place(int i, size_t o, size_t n) { off[i] = o; bytes[i] = n; }   // where someone else decided (total does not move)
  void put(int i, size_t n) { place(i, total, n); total = align_up(total + n, 256); }   // at the end: Carver::take's arithmetic
  template <typename T = float> T* at(void* base, int i) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off[i]); }
  template <typename T = float> const T* at(const void* base, int i) const {
    return reinterpret_cast<const T*>(static_cast<const char*>(base) + off[i]);
  }
};
// The plan report of the section modules (mi_fremlp_plan, mi_fourier_unit_plan, mi_sfh_ffn_plan, mi_sfh_local_plan,
// mi_sfh_global_plan, mi_sfh_mixer_plan, mi_bn2d_plan, mi_scale_res_plan), int64_t out[64]:
//   [0, FIRST)               the module's scalars, in the order the comment at its mi_*_plan lists them; the rest 0
//   [FIRST, FIRST + 2N)      (byte offset, bytes) of the N workspace sections, in the order of the module's section enum
//   [FIRST2, FIRST2 + 2M)    the same for the saved blob's sections, where the module reports them (the two mixers)
//   [60], [61], [62]         the tail: workspace bytes, the saved blob's bytes (bn2d: the stat's), one value of the module's; [63] 0
// Slots between the sets are 0.  The sets cannot overlap one another or the tail: the counts are checked where it is compiled.
template <int N> static inline void report_sections(int64_t* v, int first, const Sections<N>& s) {
  for (int i = 0; i < N; ++i) { v[first + 2 * i] = (int64_t)s.off[i]; v[first + 2 * i + 1] = (int64_t)s.bytes[i]; }
}
template <int FIRST, int S, int N>
static inline int plan_report(int64_t* out, const int64_t (&scalars)[S], const Sections<N>& ws, const int64_t (&tail)[3]) {
  static_assert(S <= FIRST && FIRST + 2 * N <= 60, "plan report: the sections overlap the scalars or reach the tail");
  memset(out, 0, 64 * sizeof(int64_t));
  for (int i = 0; i < S; ++i) out[i] = scalars[i];
  report_sections(out, FIRST, ws);
  for (int i = 0; i < 3; ++i) out[60 + i] = tail[i];
  return MI_OK;
}
template <int FIRST, int FIRST2, int S, int N, int M>
static inline int plan_report(int64_t* out, const int64_t (&scalars)[S], const Sections<N>& ws, const Sections<M>& saved,
                              const int64_t (&tail)[3]) {
  static_assert(FIRST + 2 * N <= FIRST2 && FIRST2 + 2 * M <= 60, "plan report: the saved sections overlap the workspace's or reach the tail");
  plan_report<FIRST>(out, scalars, ws, tail);
  report_sections(out, FIRST2, saved);
  return MI_OK;
}
// plain 1x1 conv: y[B,M,N] = W[M,K] x[B,K,N] (+bias) (+res);  transposed: W given as [K,M] used as its transpose.
// x_bs / y_bs: batch strides in elements where x / y are channel slices of wider tensors (0: dense, K*N / M*N).
static inline mi_pw_desc conv1x1(const void* x, int K, const float* w, bool transposed, int w_ld, const float* bias,
                                 const void* res, void* y, int M, int B, int64_t N, int dtype, int64_t x_bs = 0, int64_t y_bs = 0) {
  mi_pw_desc d;
  memset(&d, 0, sizeof(d));
  d.x1 = x; d.x1_bs = x_bs ? x_bs : (int64_t)K * N; d.k1 = K;
  d.w = w;
  if (transposed) { d.w_sm = 1; d.w_sk = w_ld; } else { d.w_sm = w_ld; d.w_sk = 1; }
  d.bias = bias;
  d.r = res; d.r_bs = (int64_t)M * N;
  d.y = y; d.y_bs = y_bs ? y_bs : (int64_t)M * N;
  d.m = M; d.n = N; d.batch = B; d.groups = 1; d.dtype = dtype;
  return d;
}
// the same with one M x K matrix per image; w_b16: optional bf16 image of the matrices as the GEMM reads them ([B][M][K])
static inline mi_pw_desc per_image(mi_pw_desc d, const void* w_b16 = nullptr) {
  d.w_bs = (int64_t)d.m * d.k1;
  if (w_b16) { d.w_b16 = w_b16; d.w_b16_sm = d.k1; }
  return d;
}
// weight gradient of a 1x1 conv: out[m,k] (+)= sum_b dy[b] x[b]^T;  sum_batch = 0: one m x k product per image instead
static inline mi_gram_desc wgrad_gram(const void* dy, int m, const void* x, int k, int B, int64_t N, int dtype, float* out,
                                      int accumulate, int sum_batch = 1, int64_t dy_bs = 0, int64_t x_bs = 0) {
  mi_gram_desc g;
  memset(&g, 0, sizeof(g));
  g.a = dy; g.a_bs = dy_bs ? dy_bs : (int64_t)m * N; g.ma = m;
  g.b = x; g.b_bs = x_bs ? x_bs : (int64_t)k * N; g.mb = k;
  g.n = N; g.batch = B; g.groups = 1; g.dtype = dtype;
  g.sum_batch = sum_batch; g.accumulate = accumulate; g.out = out; g.out_ld = k; g.out_zs = sum_batch ? 0 : (int64_t)m * k;
  return g;
}
// Workspaces are sized, and coverage is answered, before any tensor exists.  The planners (pw_plan in pw_gemm.hip, gram_plan in
// gram.hip: each the one place that decides its family's launches, and what mi_pw_gemm_workspace / mi_gram_workspace size from)
// read shapes, strides and whether the operands are 16-byte aligned, never the memory: one aligned placeholder stands in for
// every pointer.
static void* const PROBE_PTR = (void*)256;
static inline mi_pw_desc probe1x1(int K, int M, bool transposed, int B, int64_t N, int dtype, int64_t x_bs = 0, int64_t y_bs = 0) {
  return conv1x1(PROBE_PTR, K, (const float*)PROBE_PTR, transposed, transposed ? M : K, nullptr, nullptr, PROBE_PTR, M, B, N, dtype,
                 x_bs, y_bs);
}
static inline mi_gram_desc probe_wgrad(int m, int k, int B, int64_t N, int dtype, int sum_batch = 1, int64_t dy_bs = 0,
                                       int64_t x_bs = 0) {
  return wgrad_gram(PROBE_PTR, m, PROBE_PTR, k, B, N, dtype, (float*)PROBE_PTR, 0, sum_batch, dy_bs, x_bs);
}
static inline size_t pw_ws_bytes(const mi_pw_desc& d) { return mi_pw_gemm_workspace(&d); }
static inline size_t gram_ws_bytes(const mi_gram_desc& d) { return mi_gram_workspace(&d); }
// Backward of a 1x1 conv y = W x (+ b) whose input gradient leaves the module: dw (+)= sum_b dy x^T, db (+)= sum dy (optional),
// dx = W^T dy.  dy [B,M,N], x and dx [B,K,N], w [M,K].  fork: run the Gram and the bias sum beside the GEMM where MI_CO_STREAM
// asks for it (modules.hip); cross-MDTA and MEFC pass false: they never forked, and the switch must not change their streams.
__attribute__((visibility("hidden")))   // (the library's dynamic symbol list stays as it was)
int conv1x1_bwd_input(const void* dy, int M, const void* x, int K, const float* w, float* dw, float* db, void* dx, int B, int64_t N,
                      int dtype, int accumulate, void* gram_ws, void* cs_ws, void* pw_ws, hipStream_t st, bool fork);
}  // namespace mi
