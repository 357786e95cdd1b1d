// The real 2-D transforms as dense-DFT GEMMs (dft2.hip), for the modules that stand on them: the FFT loss (fftloss.hip), FreMLP
// (fremlp.hip) and FourierUnit (sfh.hip).  Host declarations only: the GEMM kernel and the table fill live in dft2.hip alone.
//
//   K = W/2 + 1,  P planes,  E_N[a][b] = exp(-2 pi i ((a b) mod N) / N)
//   rows forward    T = x . E_W            [P*H x W] real x [W x K] complex    (planes folded into the rows: the table is shared)
//   columns         Z = E_H . T  or  conj(E_H) . T   [H x H] x [H x K] complex, per plane
//   rows backward   out = scale Re(T . B)  [P*H x K] complex x [K x W] complex, real part only, rounded once
// Spectra are planar fp32 Re | Im [P][H][K]; x / out [P][H][W] in `dtype`.  Tables are rebuilt by every launch sequence.
#pragma once
#include "internal.h"

namespace mi {

constexpr int FL_MIN = 2, FL_MAX = 512;      // supported H and W
constexpr int FL_TM = 64;                    // rows per workgroup tile: four waves, one 16-row fragment each
constexpr int FL_KC = 16;                    // contraction depth per LDS stage (four k-steps of the 16x16x4 MFMA)
constexpr int FL_THREADS = 256;

// What the GEMM stages of one (P, H, W) run on: filled by dft2_geom, the ONE place that decides tiles and grids.
struct Dft2Geom {
  int P, H, W, K;
  int nf_l, nf_x;                    // 16-column fragments per tile over l (width K) and over x (width W): 3, 4 or 5
  int l_blocks, x_blocks;            // tiles over K and over W
  int m_tiles_fold, m_tiles_plane;   // 64-row tiles over P*H (the rows stages) and over H (the columns stage: one set per plane)
  int grid_tab, grid_fold_l, grid_plane, grid_fold_x;   // table fill; [P*H] x K tiles; per-plane H x K tiles; [P*H] x W tiles
};
// false (and *g zero): H or W outside FL_MIN..FL_MAX, P < 1, or too many planes for a grid
MI_HIDDEN bool dft2_geom(int64_t P, int H, int W, Dft2Geom* g);

// cos | sin of E_W [W][K], their transposes [K][W], the same four with the c2r column weights w_l folded in (w_l = 1 at l = 0
// and, for even W, l = W/2, else 2), cos | sin of E_H [H][H]
enum { DT_CW = 0, DT_SW, DT_CWT, DT_SWT, DT_WCW, DT_WSW, DT_WCWT, DT_WSWT, DT_CH, DT_SH, DFT2_TABLES };
static inline size_t dft2_table_bytes(const Dft2Geom& g, int i) { return (i < DT_CH ? (size_t)g.W * g.K : (size_t)g.H * g.H) * 4; }
// The tables and the one complex [P*H][K] intermediate (re, im) the directions below pass through.  The four weighted tables may
// be null where only the stages are used (the FFT loss has no such sections).
struct Dft2Ws { float* tab[DFT2_TABLES]; float* tre; float* tim; };
MI_HIDDEN int dft2_tables(const Dft2Geom& g, const Dft2Ws& w, hipStream_t st);

// The transform's own blob, mi_dft2_workspace() bytes: the ten tables in the order above, then the complex intermediate, every
// section 256-byte aligned.  A module that embeds the blob in its workspace takes the layout from here.
struct Dft2Blob { size_t tab[DFT2_TABLES], t, total; int64_t bins; };   // byte offsets of the tables, of the intermediate (= the tables'
                                                                         // share); size; P H K
MI_HIDDEN bool dft2_blob(const Dft2Geom& g, Dft2Blob* b);   // false: more than INT_MAX bins (modules index a spectrum with int)
MI_HIDDEN Dft2Ws dft2_blob_ws(const Dft2Blob& b, void* base);

// ---- the stages ----
// [P*H x W] real (activation dtype; sub != null: x - sub, widened first) . (tc - i ts) [W][K] -> ore | oim
MI_HIDDEN int dft2_rows_fwd(const Dft2Geom& g, const void* x, const void* sub, const float* tc, const float* ts, float* ore, float* oim,
                            int dtype, hipStream_t st);
// per plane: (cos H + i sign sin H) . in -> out;  sign -1: E_H, +1: conj(E_H)
MI_HIDDEN int dft2_cols(const Dft2Geom& g, const Dft2Ws& w, float sign, const float* ire, const float* iim, float* ore, float* oim,
                        hipStream_t st);
// per plane: Z = E_H . in, never stored: sre | sim = sign(Re Z) | sign(Im Z) (skipped when null) and one |Re| + |Im| sum per
// workgroup, part[grid_plane]
MI_HIDDEN int dft2_cols_sign(const Dft2Geom& g, const Dft2Ws& w, const float* ire, const float* iim, float* sre, float* sim, float* part,
                             hipStream_t st);
// out = scale * Re(in . (tc + i ts) [K][W]), rounded once to the activation dtype
MI_HIDDEN int dft2_rows_bwd(const Dft2Geom& g, const float* ire, const float* iim, const float* tc, const float* ts, void* out, float scale,
                            int dtype, hipStream_t st);

// ---- the four directions, each two stages through w.tre | w.tim (no operand may lie there) ----
MI_HIDDEN int dft2_r2c_run(const Dft2Geom& g, const Dft2Ws& w, const void* x, float* zre, float* zim, int dtype, hipStream_t st);   // Z = rfft2(x)
MI_HIDDEN int dft2_c2r_run(const Dft2Geom& g, const Dft2Ws& w, const float* yre, const float* yim, void* out, int dtype, hipStream_t st);   // irfft2(Y, norm='backward')
MI_HIDDEN int dft2_c2r_adj(const Dft2Geom& g, const Dft2Ws& w, const void* dout, float* gre, float* gim, int dtype, hipStream_t st);   // H W x the adjoint of c2r
MI_HIDDEN int dft2_r2c_adj(const Dft2Geom& g, const Dft2Ws& w, const float* dre, const float* dim, void* dx, int dtype, hipStream_t st);   // the adjoint of r2c

}  // namespace mi
