// Row-Gram contraction over the pixel axis:  G[z][i][j] = sum_n A[z][i][n] * Bm[z][j][n].
// This one kernel is MDTA's q k^T (Restormer.py:124, with the F.normalize row sums of squares of
// :121-122 taken from the same operand fragments), the per-image dY V^T of its backward, and every
// 1x1-conv weight gradient (sum over batch).  Both operands are pixel-contiguous, so both MFMA
// fragments are plain 16-byte row reads from LDS.  The pixel axis is split across workgroups; partial
// tiles go to a workspace and are summed in a fixed order by a second kernel (bitwise reproducible).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "internal.h"

namespace mi {

struct GramK {
  const void* a; int64_t a_bs, a_gs; int ma;
  const void* b; int64_t b_bs, b_gs; int mb;
  int64_t n; int groups; int Z;
  float* part;     // [splits][Z][ma][mb]
  float* ss_part;  // [splits][Z][ma+mb] or null
  int chunks_per_split, nchunks, tiles_b, vec_ok;
  int fold;        // > 0: the batch is folded into the pixel axis (weight gradients): chunk / step c lies in image c / fold
};

template <typename T, int FA, int FB, bool SS>   // tile = (32 FA) rows of A x (32 FB) rows of B; the 2 x 2 waves own 16 FA x 16 FB fragments each
__global__ __launch_bounds__(256) void gram_kernel(GramK p) {
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int TA = 32 * FA, TB = 32 * FB;
  constexpr int KC = F32 ? 32 : 64;        // pixels per staged chunk (128 bytes per row)
  constexpr int AS = F32 ? 34 : 72;        // LDS row stride, elements
  constexpr int EPV = F32 ? 4 : 8;         // elements per 16-byte vector
  __shared__ __attribute__((aligned(16))) T As[TA * AS];
  __shared__ __attribute__((aligned(16))) T Bs[TB * AS];

  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);   // (scalar wave index)
  const int li = lane & 15, g = lane >> 4;
  const int wr = wv >> 1, wc = wv & 1;
  const int z = blockIdx.z, zb = p.fold ? 0 : z / p.groups, zg = p.fold ? z : z - zb * p.groups;
  const int ta = blockIdx.y / p.tiles_b, tb = blockIdx.y - ta * p.tiles_b;
  const int i0 = ta * TA, j0 = tb * TB;
  const T* A = (const T*)p.a + zb * p.a_bs + zg * p.a_gs;
  const T* B = (const T*)p.b + zb * p.b_bs + zg * p.b_gs;
  const int c_begin = blockIdx.x * p.chunks_per_split;
  int c_end = c_begin + p.chunks_per_split;
  if (c_end > p.nchunks) c_end = p.nchunks;

  u32x4 areg[FA], breg[FB];
  // (thread / lane ids below are opaque copies: the per-lane address terms are loop-invariant, and kept across the chunk loop
  //  they are what lifts this kernel over the 170 registers that allow a third workgroup per CU)
  auto load_rows = [&](auto cnt, const T* base, int64_t img_stride, int row0, int rows, int chunk, u32x4* regs) {
    constexpr int F = decltype(cnt)::value;
    int tt = t;
    asm volatile("" : "+v"(tt));
    if (p.fold) {                                                    // (uniform) image of this chunk, chunk inside the image
      const int img = chunk / p.fold;
      base += img * img_stride;
      chunk -= img * p.fold;
    }
#pragma unroll
    for (int i = 0; i < F; ++i) {
      const int v = tt + 256 * i;
      const int row = v >> 3, seg = v & 7;
      const int64_t n = (int64_t)chunk * KC + seg * EPV;
      const int r = row0 + row;
      if (r < rows && p.vec_ok && n < p.n) {
        regs[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)r * p.n + n);
      } else {
        __attribute__((aligned(16))) T tmp[EPV];
#pragma unroll
        for (int e = 0; e < EPV; ++e) tmp[e] = (r < rows && n + e < p.n) ? base[(int64_t)r * p.n + n + e] : Cvt<T>::from(0.f);
        regs[i] = *reinterpret_cast<u32x4*>(tmp);
      }
    }
  };
  auto write_rows = [&](auto cnt, T* dst, const u32x4* regs) {
    constexpr int F = decltype(cnt)::value;
    int tt = t;
    asm volatile("" : "+v"(tt));
#pragma unroll
    for (int i = 0; i < F; ++i) {
      const int v = tt + 256 * i;
      const int row = v >> 3, seg = v & 7;
      T* d = dst + row * AS + seg * EPV;
      if constexpr (F32) {  // 136-byte rows: 8-byte aligned only
        *reinterpret_cast<u32x2*>(d) = (u32x2){regs[i][0], regs[i][1]};
        *reinterpret_cast<u32x2*>(d + 2) = (u32x2){regs[i][2], regs[i][3]};
      } else {
        *reinterpret_cast<u32x4*>(d) = regs[i];
      }
    }
  };

  constexpr std::integral_constant<int, FA> NA{};
  constexpr std::integral_constant<int, FB> NB{};
  f32x4 acc[FA][FB];
  float ssa[FA], ssb[FB];
#pragma unroll
  for (int a = 0; a < FA; ++a) {
    ssa[a] = 0.f;
#pragma unroll
    for (int b = 0; b < FB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int b = 0; b < FB; ++b) ssb[b] = 0.f;
  const int ra = wr * 16 * FA, cb = wc * 16 * FB;  // wave's first row / col inside the tile

  if (c_begin < c_end) {
    load_rows(NA, A, p.a_bs, i0, p.ma, c_begin, areg);
    load_rows(NB, B, p.b_bs, j0, p.mb, c_begin, breg);
  }
  for (int c = c_begin; c < c_end; ++c) {
    __syncthreads();
    write_rows(NA, As, areg);
    write_rows(NB, Bs, breg);
    __syncthreads();
    if (c + 1 < c_end) {
      load_rows(NA, A, p.a_bs, i0, p.ma, c + 1, areg);
      load_rows(NB, B, p.b_bs, j0, p.mb, c + 1, breg);
    }
    if constexpr (F32) {
#pragma unroll
      for (int ks = 0; ks < KC / 4; ++ks) {
        const int kk = 4 * ks + g;
        float av[FA], bv[FB];
#pragma unroll
        for (int f = 0; f < FA; ++f) {
          av[f] = As[(ra + 16 * f + li) * AS + kk];
          if (SS) ssa[f] += av[f] * av[f];
        }
#pragma unroll
        for (int f = 0; f < FB; ++f) {
          bv[f] = Bs[(cb + 16 * f + li) * AS + kk];
          if (SS) ssb[f] += bv[f] * bv[f];
        }
#pragma unroll
        for (int fa = 0; fa < FA; ++fa)
#pragma unroll
          for (int fb = 0; fb < FB; ++fb)
            acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[fa], bv[fb], acc[fa][fb], 0, 0, 0);
      }
    } else {
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const T* ap = &As[(ra + (ln & 15)) * AS + 8 * (ln >> 4)];
      const T* bp = &Bs[(cb + (ln & 15)) * AS + 8 * (ln >> 4)];
#pragma unroll
      for (int ks = 0; ks < KC / 32; ++ks) {
        s16x8 av[FA], bv[FB];
#pragma unroll
        for (int f = 0; f < FA; ++f) {
          av[f] = *reinterpret_cast<const s16x8*>(ap + 16 * f * AS + 32 * ks);
          if (SS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float x = bf16_bits_to_f32((unsigned int)(unsigned short)av[f][e]);
              ssa[f] += x * x;
            }
          }
        }
#pragma unroll
        for (int f = 0; f < FB; ++f) {
          bv[f] = *reinterpret_cast<const s16x8*>(bp + 16 * f * AS + 32 * ks);
          if (SS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float y = bf16_bits_to_f32((unsigned int)(unsigned short)bv[f][e]);
              ssb[f] += y * y;
            }
          }
        }
#pragma unroll
        for (int fa = 0; fa < FA; ++fa)
#pragma unroll
          for (int fb = 0; fb < FB; ++fb)
            acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[fa], bv[fb], acc[fa][fb], 0, 0, 0);
      }
    }
  }

  // lane holds G[i0+ra+16fa+4g+r][j0+cb+16fb+li]
  float* pz = p.part + ((int64_t)blockIdx.x * p.Z + z) * ((int64_t)p.ma * p.mb);
#pragma unroll
  for (int fa = 0; fa < FA; ++fa)
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      const int j = j0 + cb + 16 * fb + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + ra + 16 * fa + 4 * g + r;
        if (i < p.ma && j < p.mb) pz[(int64_t)i * p.mb + j] = acc[fa][fb][r];
      }
    }
  if (SS && p.ss_part) {
    float* sz = p.ss_part + ((int64_t)blockIdx.x * p.Z + z) * (p.ma + p.mb);
#pragma unroll
    for (int f = 0; f < FA; ++f) {
      float sa = ssa[f];
      sa += __shfl_xor(sa, 16, 64); sa += __shfl_xor(sa, 32, 64);
      const int i = i0 + ra + 16 * f + li;
      if (g == 0 && wc == 0 && tb == 0 && i < p.ma) sz[i] = sa;
    }
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      float sb = ssb[f];
      sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
      const int j = j0 + cb + 16 * f + li;
      if (g == 0 && wr == 0 && ta == 0 && j < p.mb) sz[p.ma + j] = sb;
    }
  }
}

// ---- bf16 streaming form ------------------------------------------------------------------------------------------------
// Both operands are pixel-contiguous, and the MFMA k index may be ANY permutation of the pixels as long as A and B use
// the same one - so a lane's fragment (row li, 8 consecutive pixels) is one plain 16-byte global load and nothing needs
// LDS.  A wave owns the whole (16 FA) x (16 FB) tile over its own pixels: per 64-pixel step it loads the two halves of
// one 128-byte line of each row (k-steps 0 and 1) and issues 2 FA FB MFMAs, with the next step's (FA + FB) x 2 loads
// already in flight; the four waves of a workgroup take interleaved steps of the workgroup's pixel range and are summed
// in a fixed order through LDS at the end.  No barrier in the streaming loop (the LDS-staged kernel above: two per chunk).
template <int FA, int FB, bool SS>
__global__ __launch_bounds__(256) void gram_stream_kernel(GramK p, int steps_per_block, int nsteps) {
  using T = bf16;
  __shared__ __attribute__((aligned(16))) f32x4 red[2][FA * FB][64];
  __shared__ float ssm[SS ? 4 : 1][SS ? (FA + FB) * 16 : 1];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);   // (scalar wave index)
  const int li = lane & 15, g = lane >> 4;
  const int z = blockIdx.z, zb = p.fold ? 0 : z / p.groups, zg = p.fold ? z : z - zb * p.groups;
  const int ta = blockIdx.y / p.tiles_b, tb = blockIdx.y - ta * p.tiles_b;
  const int i0 = ta * 16 * FA, j0 = tb * 16 * FB;
  const T* A0 = (const T*)p.a + zb * p.a_bs + zg * p.a_gs;
  const T* B0 = (const T*)p.b + zb * p.b_bs + zg * p.b_gs;
  const int s_begin = blockIdx.x * steps_per_block;
  const int s_end = min(s_begin + steps_per_block, nsteps);

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // Row addresses are rebuilt for every step from an opaque copy of the lane id: kept across the loop (FA + FB 64-bit pointers
  // and their validity flags) they cost ~30 registers of a kernel that needs every one for its two steps of loads in flight.
  auto load_step = [&](int s, u32x4 (*av)[2], u32x4 (*bv)[2]) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int li_ = ln & 15, g_ = ln >> 4;
    // 32-bit element offsets from the (uniform) operand bases: one slice is at most rows * n < 2^31 elements (gram_plan)
    const T* A = A0;
    const T* B = B0;
    int sl = s;                                          // step inside its image
    if (p.fold) {
      const int img = s / p.fold;
      sl = s - img * p.fold;
      A += img * p.a_bs; B += img * p.b_bs;
    }
    const unsigned px = (unsigned)sl * 64u + 8u * g_;    // this lane's first pixel of k-step 0; k-step 1 is 32 further
    const unsigned un = (unsigned)p.n;
    const bool in0 = s < s_end && px + 8 <= un, in1 = s < s_end && px + 40 <= un;
#pragma unroll
    for (int f = 0; f < FA; ++f) {
      const int r = i0 + 16 * f + li_;
      const bool ok = r < p.ma;
      const u32x4* q = reinterpret_cast<const u32x4*>(A + ((unsigned)(ok ? r : 0) * un + px));
      av[f][0] = (ok && in0) ? q[0] : zero4;
      av[f][1] = (ok && in1) ? q[4] : zero4;
    }
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      const int r = j0 + 16 * f + li_;
      const bool ok = r < p.mb;
      const u32x4* q = reinterpret_cast<const u32x4*>(B + ((unsigned)(ok ? r : 0) * un + px));
      bv[f][0] = (ok && in0) ? q[0] : zero4;
      bv[f][1] = (ok && in1) ? q[4] : zero4;
    }
  };

  f32x4 acc[FA][FB];
  float ssa[FA], ssb[FB];
#pragma unroll
  for (int a = 0; a < FA; ++a) {
    ssa[a] = 0.f;
#pragma unroll
    for (int b = 0; b < FB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int b = 0; b < FB; ++b) ssb[b] = 0.f;

  u32x4 ca[FA][2], cb[FB][2];
  load_step(s_begin + wv, ca, cb);
  for (int s = s_begin + wv; s < s_end; s += 4) {
    u32x4 na[FA][2], nb[FB][2];
    load_step(s + 4, na, nb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s16x8 av[FA], bv[FB];
#pragma unroll
      for (int f = 0; f < FA; ++f) av[f] = __builtin_bit_cast(s16x8, ca[f][h]);
#pragma unroll
      for (int f = 0; f < FB; ++f) bv[f] = __builtin_bit_cast(s16x8, cb[f][h]);
      if (SS) {
#pragma unroll
        for (int f = 0; f < FA; ++f)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = bf16_bits_to_f32((unsigned int)(unsigned short)av[f][e]);
            ssa[f] += x * x;
          }
#pragma unroll
        for (int f = 0; f < FB; ++f)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float y = bf16_bits_to_f32((unsigned int)(unsigned short)bv[f][e]);
            ssb[f] += y * y;
          }
      }
#pragma unroll
      for (int fa = 0; fa < FA; ++fa)
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
          acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[fa], bv[fb], acc[fa][fb], 0, 0, 0);
    }
#pragma unroll
    for (int f = 0; f < FA; ++f) { ca[f][0] = na[f][0]; ca[f][1] = na[f][1]; }
#pragma unroll
    for (int f = 0; f < FB; ++f) { cb[f][0] = nb[f][0]; cb[f][1] = nb[f][1]; }
  }

  // fixed-order sum of the four waves: (w0 + w2) + (w1 + w3)
  if (wv >= 2) {
#pragma unroll
    for (int fa = 0; fa < FA; ++fa)
#pragma unroll
      for (int fb = 0; fb < FB; ++fb) red[wv - 2][fa * FB + fb][lane] = acc[fa][fb];
  }
  if (SS) {
#pragma unroll
    for (int f = 0; f < FA; ++f) {
      float v = ssa[f];
      v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      if (g == 0) ssm[wv][16 * f + li] = v;
    }
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      float v = ssb[f];
      v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      if (g == 0) ssm[wv][16 * (FA + f) + li] = v;
    }
  }
  __syncthreads();
  if (wv < 2) {
#pragma unroll
    for (int fa = 0; fa < FA; ++fa)
#pragma unroll
      for (int fb = 0; fb < FB; ++fb) {
        const f32x4 o = red[wv][fa * FB + fb][lane];
        acc[fa][fb] += o;
      }
  }
  __syncthreads();
  if (wv == 1) {
#pragma unroll
    for (int fa = 0; fa < FA; ++fa)
#pragma unroll
      for (int fb = 0; fb < FB; ++fb) red[0][fa * FB + fb][lane] = acc[fa][fb];
  }
  __syncthreads();
  if (wv != 0) return;
  float* pz = p.part + ((int64_t)blockIdx.x * p.Z + z) * ((int64_t)p.ma * p.mb);
#pragma unroll
  for (int fa = 0; fa < FA; ++fa)
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
      const f32x4 o = acc[fa][fb] + red[0][fa * FB + fb][lane];
      const int j = j0 + 16 * fb + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * fa + 4 * g + r;
        if (i < p.ma && j < p.mb) pz[(int64_t)i * p.mb + j] = o[r];
      }
    }
  if (SS && p.ss_part) {
    float* sz = p.ss_part + ((int64_t)blockIdx.x * p.Z + z) * (p.ma + p.mb);
    for (int e = lane; e < (FA + FB) * 16; e += 64) {
      const float v = (ssm[0][e] + ssm[2][e]) + (ssm[1][e] + ssm[3][e]);
      if (e < FA * 16) { const int i = i0 + e; if (tb == 0 && i < p.ma) sz[i] = v; }
      else { const int j = j0 + e - FA * 16; if (ta == 0 && j < p.mb) sz[p.ma + j] = v; }
    }
  }
}

// out[zo][i*ld + j] (+)= sum_{split} sum_{b if sum_batch} part[split][b*groups+g][i][j]
// 256 threads = 16 consecutive elements x 16 slice-phases; each thread walks its slices 4 at a time (loads in flight),
// phases are combined through LDS in a fixed order (reproducible).
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                          int splits, int batch, int groups, int ma, int mb, int64_t out_ld,
                                                          int64_t out_zs, int sum_batch, int accumulate) {
  __shared__ float sm[16][17];
  const int ex = threadIdx.x & 15, ph = threadIdx.x >> 4;
  const int64_t e = (int64_t)blockIdx.x * 16 + ex;
  const int64_t per = (int64_t)ma * mb;
  const int zo = blockIdx.y;
  const int Z = batch * groups;
  const int nb = sum_batch ? batch : 1;
  const int total = splits * nb;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < per) {
    auto addr = [&](int q) -> int64_t {
      const int sp = q / nb, b = q - sp * nb;
      const int64_t zz = sum_batch ? ((int64_t)b * groups + zo) : zo;
      return ((int64_t)sp * Z + zz) * per + e;
    };
    int q = ph;
    for (; q + 48 < total; q += 64) {
      s0 += part[addr(q)]; s1 += part[addr(q + 16)]; s2 += part[addr(q + 32)]; s3 += part[addr(q + 48)];
    }
    for (; q < total; q += 16) s0 += part[addr(q)];
  }
  sm[ph][ex] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ph == 0 && e < per) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sm[k][ex];
    const int i = (int)(e / mb), j = (int)(e - (int64_t)i * mb);
    float* o = out + (int64_t)zo * out_zs + (int64_t)i * out_ld + j;
    *o = (accumulate ? *o : 0.f) + s;
  }
}

// Few slices, or enough output elements to fill the chip: one thread per output element, the slices walked in order NS at a time
// (the 16-phase kernel above keeps 1/16 of its lanes busy there: 33 us for 43 MB at C = 384, profiles/r04_f_attn_small.txt).
template <int NS>
__global__ __launch_bounds__(256) void gram_reduce_few_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                              int total, int batch, int groups, int ma, int mb, int64_t out_ld,
                                                              int64_t out_zs, int sum_batch, int accumulate) {
  const int64_t per = (int64_t)ma * mb;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int zo = blockIdx.y;
  if (e >= per) return;
  const int Z = batch * groups;
  const int nb = sum_batch ? batch : 1;
  float s = 0.f;
  for (int q0 = 0; q0 < total; q0 += NS) {       // NS loads in flight, summed in slice order
    float v[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int q = q0 + u;
      const int sp = q / nb, b = q - sp * nb;
      const int64_t zz = sum_batch ? ((int64_t)b * groups + zo) : zo;
      v[u] = q < total ? part[((int64_t)sp * Z + zz) * per + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) s += v[u];
  }
  const int i = (int)(e / mb), j = (int)(e - (int64_t)i * mb);
  float* o = out + (int64_t)zo * out_zs + (int64_t)i * out_ld + j;
  *o = (accumulate ? *o : 0.f) + s;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// Weight gradients sum over the batch: instead of one partial tile per image (and a reduction over batch x splits partials),
// the images are chained along the contraction axis - a workgroup's pixel range may cross image boundaries - whenever an image
// is a whole number of chunks / steps.  Returns the chunks per image, or 0.  Measured at bs 32 (profiles/r02_k_gram_fold_ab.txt):
// it pays where an image is short (32 x 32 planes: 16 chunks per workgroup against a 64 KB partial tile each - 1152 x 384
// 102 -> 76 us, 2042 x 384 144 -> 127 us) and where images x tiles leaves the chip half empty (576 x 192 at 64 x 64: 320
// workgroups, 163 -> 125 us); on long planes the per-chunk image lookup costs 5-10 % and buys nothing, so those stay per image.
// sw: MI_GRAM_FOLD (A/B switch: 0 never, 2 wherever possible).
static int gram_fold(const mi_gram_desc* d, int unit, int64_t tiles_per_image, const char* sw) {
  if (sw && sw[0] == '0') return 0;
  if (!d->sum_batch || d->batch <= 1 || d->sumsq || d->n % unit != 0 || d->n / unit > (1 << 20)) return 0;
  // (second case: the per-image plan would run ONE split - 512 / workgroups rounds to 1 - on a chip it does not fill)
  const int64_t wgs = tiles_per_image * d->batch;
  const bool pays = d->n / unit <= 16 || (wgs > 256 && wgs < 448);
  if (!pays && !(sw && sw[0] == '2')) return 0;
  return (int)(d->n / unit);
}
// streaming form: 16-row fragments per tile side, the count that pads the rows least (ties: the larger tile)
static int gram_pick_frags(int m) {
  int best = 3, best_pad = 1 << 30;
  for (int f : {3, 4, 6}) {
    const int pad = cdiv(m, 16 * f) * 16 * f;
    if (pad < best_pad || (pad == best_pad && f > best)) { best = f; best_pad = pad; }
  }
  return best;
}

// What one call runs (GramPlan, internal.h).  The ONE place that decides it, and the only reader of the MI_GRAM_* switches (each
// read once): mi_gram launches what it says, mi_gram_workspace sizes from it, mi_gram_plan reports it.  Pointers are read for
// their alignment only.  force = GRAM_LDS / GRAM_STREAM: the plan of that family whatever dtype, alignment, switches and
// thresholds say - for sizing only (workspaces are sized before the pointers exist), never launched.
static GramPlan gram_plan(const mi_gram_desc* d, int force = -1) {
  GramPlan g{};
  const bool bf = d->dtype == MI_BF16;
  const char* fold_sw = MI_ENV(MI_GRAM_FOLD);
  const char* want_sw = MI_ENV(MI_GRAM_WANT);                       // A/B switch: workgroups the pixel split aims for
  const char* rect_sw = MI_ENV(MI_GRAM_RECT);                       // MI_GRAM_RECT=0: square tiles only (A/B switch)
  const bool rect = bf && !(rect_sw && rect_sw[0] == '0');
  const int64_t vec = bf ? 8 : 4;
  g.vec_ok = d->n % vec == 0 && aligned16(d->a) && aligned16(d->b) && d->a_bs % vec == 0 && d->a_gs % vec == 0 && d->b_bs % vec == 0 &&
             d->b_gs % vec == 0;
  g.ss = d->sumsq != nullptr;
  // ---- the LDS-staged tile: 32-row fragments per side
  int la, lb;
  la = lb = (d->ma > 64 || d->mb > 64) ? 4 : 2;
  // rectangular tiles (bf16): a tile that holds ALL of the shorter operand's rows reads the other operand once instead of once
  // per 128-row tile of it - 96 x 255 (project_out's weight gradient) as ONE 96 x 256 tile, M x 192 (the C = 192 level) and the
  // wide M x 384 as 128 x 192 tiles.  bs 32 (profiles/r02_o_gram_rect_tiles.txt): 96 x 255 at 256^2 343 -> 304 us, 1020 x 192
  // 158 -> 116, 576 x 192 124 -> 85, 2042 x 384 128 -> 105 (384 x 384 loses: 35 -> 39, stays square); step 153.6 -> 152.1 ms.
  if (rect && d->ma > 64 && d->ma <= 96 && d->mb > 64 && d->mb <= 96) {
    la = lb = 3;                                                     // 96 x 96 (q k^T and dM at c = 96): no padded fragments
  } else if (rect && !g.ss) {
    if (d->ma <= 96 && d->mb > 128 && d->mb <= 256) { la = 3; lb = 8; }
    else if (d->ma > 128 && d->mb > 128 && (d->mb <= 192 || (d->mb == 384 && d->ma > 384))) { la = 4; lb = 6; }
    else if ((d->ma > 128 && d->ma <= 192 && d->mb > 192) || (d->ma == 384 && d->mb > 384)) { la = 6; lb = 4; }   // 192 x 510 (86 -> 65 us), 384 x 1021 (71 -> 62)
  }
  // ---- the streaming tile: 16-row fragments per side
  int sa = gram_pick_frags(d->ma), sb = gram_pick_frags(d->mb);
  if (sa * sb > 24) { if (sa >= sb) sa = 3; else sb = 3; }          // 6x6 -> 3x6: accumulators + two stages of loads <= 256 VGPRs
  const int sfold = gram_fold(d, 64, 0, fold_sw);                    // (streaming form: short planes only)
  // ---- the family.  Streaming: bf16 with 16-byte rows, and a slice its 32-bit element offsets can address
  g.family = GRAM_LDS;
  if (force >= 0) {
    g.family = force;
  } else if (bf && g.vec_ok && !MI_ENV(MI_GRAM_LDS) && (int64_t)std::max(d->ma, d->mb) * d->n < (1ll << 31)) {
    // Measured (profiles/r01_s_gram_microbench.log): the streaming form wins while one or a few SMALL tiles cover the
    // output (48x48 q k^T, the 144/254/127 x 48 weight gradients: 1.1-1.7x); with 96-wide or many tiles the operand
    // re-reads and 1-wave occupancy lose to the LDS-staged 128x128 tiles (0.6-0.85x).
    // ... and where the 128 x 128 LDS tiles would be mostly padding (288 x 96 fills 56% of 3 x 1 tiles: streaming 1.27x
    // faster at bs 32; 96 x 255 and 510 x 96 fill 75% and stay on the LDS kernel; profiles/r01_y_gram_bs32.log)
    const double lds_fill = (double)d->ma * d->mb / ((double)cdiv(d->ma, 32 * la) * 32 * la * cdiv(d->mb, 32 * lb) * 32 * lb);   // (the tile the LDS kernel would actually use)
    bool stream;
    if (MI_ENV(MI_GRAM_STREAM_ALL)) stream = true;                   // A/B switch
    else if ((sfold ? (int64_t)d->batch * d->n : d->n) < 4096) stream = false;
    else if (sa <= 4 && sb <= 4 && cdiv(d->ma, 16 * sa) * cdiv(d->mb, 16 * sb) <= 4) stream = true;
    else stream = (d->ma > 64 || d->mb > 64) && lds_fill < 0.6;
    if (stream) g.family = GRAM_STREAM;
  }
  // ---- the instance and the pixel split
  const bool stream = g.family == GRAM_STREAM;
  g.fa = stream ? sa : la;
  g.fb = stream ? sb : lb;
  g.unit = stream || bf ? 64 : 32;                                   // a streaming step / a staged chunk of 128 bytes per row
  g.tiles_a = cdiv(d->ma, (stream ? 16 : 32) * g.fa);
  g.tiles_b = cdiv(d->mb, (stream ? 16 : 32) * g.fb);
  g.fold = stream ? sfold : gram_fold(d, g.unit, (int64_t)g.tiles_a * g.tiles_b * d->groups, fold_sw);
  g.Z = (g.fold ? 1 : d->batch) * d->groups;
  g.units = g.fold ? d->batch * g.fold : cdiv(d->n, g.unit);
  const int64_t tiles = (int64_t)g.tiles_a * g.tiles_b * g.Z;
  int64_t want = (want_sw ? atoi(want_sw) : (stream ? 768 : 512)) / (tiles > 0 ? tiles : 1);
  if (stream) {
    const int64_t cap = g.units / 32 > 0 ? g.units / 32 : 1;         // >= 8 steps per wave: the prefetch pipeline needs a run
    want = std::max<int64_t>(std::min(want, cap), 1);
    // several tiles re-read the same pixels: a split count that is a multiple of 8 puts them on one XCD (shared L2)
    if (g.tiles_a * g.tiles_b > 1 && want >= 8) want = want / 8 * 8;
    g.per_split = (int)((cdiv(g.units, want) + 3) / 4 * 4);
  } else {
    want = std::min<int64_t>(std::max<int64_t>(want, 1), g.units);
    g.per_split = cdiv(g.units, want);
  }
  g.splits = cdiv(g.units, g.per_split);
  g.grid = dim3(g.splits, g.tiles_a * g.tiles_b, g.Z);
  g.block = dim3(256);
  g.part_bytes = align_up((size_t)g.splits * g.Z * d->ma * d->mb * sizeof(float), 256);
  g.ss_bytes = align_up((size_t)g.splits * g.Z * (d->ma + d->mb) * sizeof(float), 256);
  // ---- how the launch finishes.  One split, one output slice per z, plain overwrite into a dense [Z][ma][mb] output: the
  // kernel's "partial" IS the result, so it writes straight to the output and the reduce launch disappears (dM = dy v^T at
  // C = 384: a 19 MB copy at 330 GB/s).  Else the partials are summed per output element, `total` of them in slice order:
  // few slices, or enough output elements to fill the chip with one thread each, by the kernel that walks them in the thread.
  const int64_t per = (int64_t)d->ma * d->mb;
  g.images = g.fold ? 1 : d->batch;
  g.total = g.splits * (d->sum_batch ? g.images : 1);
  g.zo = d->sum_batch ? d->groups : g.Z;
  if (g.splits == 1 && !d->sum_batch && !d->accumulate && d->out_ld == d->mb && d->out_zs == per) g.finish = GRAM_DIRECT;
  else if (g.total <= 4) g.finish = GRAM_REDUCE_FEW4;
  else if (g.total <= 16 || per * g.zo >= 16384) g.finish = GRAM_REDUCE_FEW16;
  else g.finish = GRAM_REDUCE;
  // A weight-gradient Gram that accumulates into a dense [ma][mb] gradient may leave its split partials in the deferred arena
  // and have them summed by mi_deferred_flush (common.h): rows = splits x images of ma*mb floats, a plain fixed-order row sum.
  g.deferrable = g.finish != GRAM_DIRECT && d->accumulate && d->sum_batch && d->groups == 1 && d->out_ld == d->mb && !g.ss;
  return g;
}

static int gram_check(const mi_gram_desc* d) {
  MI_CHECK_ARG(d && d->a && d->b && d->out, "gram: null pointer");
  MI_CHECK_ARG(d->ma > 0 && d->mb > 0 && d->n > 0 && d->batch > 0 && d->groups > 0, "gram: bad shape");
  MI_CHECK_ARG(d->dtype == MI_F32 || d->dtype == MI_BF16, "gram: bad dtype %d", d->dtype);
  MI_CHECK_ARG(d->out_ld >= d->mb, "gram: out_ld < mb");
  MI_CHECK_ARG(!(d->sumsq && d->sum_batch), "gram: sumsq with sum_batch is not supported");
  return MI_OK;
}

// ---- the instances of each family, keyed on (dtype, fa, fb); fn[1]: with the row sums of squares.  The rectangular LDS tiles
// have none: gram_plan gives them to calls without sumsq only.
using GramFn = void (*)(GramK);
using GramSFn = void (*)(GramK, int, int);
template <typename Fn> struct GramInst { int dtype, fa, fb; Fn fn[2]; };
static const GramInst<GramFn> GRAM_LDS_TABLE[] = {
    {MI_F32, 2, 2, {gram_kernel<float, 2, 2, false>, gram_kernel<float, 2, 2, true>}},
    {MI_F32, 4, 4, {gram_kernel<float, 4, 4, false>, gram_kernel<float, 4, 4, true>}},
    {MI_BF16, 2, 2, {gram_kernel<bf16, 2, 2, false>, gram_kernel<bf16, 2, 2, true>}},
    {MI_BF16, 3, 3, {gram_kernel<bf16, 3, 3, false>, gram_kernel<bf16, 3, 3, true>}},
    {MI_BF16, 4, 4, {gram_kernel<bf16, 4, 4, false>, gram_kernel<bf16, 4, 4, true>}},
    {MI_BF16, 3, 8, {gram_kernel<bf16, 3, 8, false>, nullptr}},
    {MI_BF16, 4, 6, {gram_kernel<bf16, 4, 6, false>, nullptr}},
    {MI_BF16, 6, 4, {gram_kernel<bf16, 6, 4, false>, nullptr}}};
static const GramInst<GramSFn> GRAM_STREAM_TABLE[] = {
    {MI_BF16, 3, 3, {gram_stream_kernel<3, 3, false>, gram_stream_kernel<3, 3, true>}},
    {MI_BF16, 3, 4, {gram_stream_kernel<3, 4, false>, gram_stream_kernel<3, 4, true>}},
    {MI_BF16, 3, 6, {gram_stream_kernel<3, 6, false>, gram_stream_kernel<3, 6, true>}},
    {MI_BF16, 4, 3, {gram_stream_kernel<4, 3, false>, gram_stream_kernel<4, 3, true>}},
    {MI_BF16, 4, 4, {gram_stream_kernel<4, 4, false>, gram_stream_kernel<4, 4, true>}},
    {MI_BF16, 4, 6, {gram_stream_kernel<4, 6, false>, gram_stream_kernel<4, 6, true>}},
    {MI_BF16, 6, 3, {gram_stream_kernel<6, 3, false>, gram_stream_kernel<6, 3, true>}},
    {MI_BF16, 6, 4, {gram_stream_kernel<6, 4, false>, gram_stream_kernel<6, 4, true>}}};
template <typename Fn, size_t N> static Fn gram_find(const GramInst<Fn> (&tab)[N], int dtype, const GramPlan& g) {
  for (const GramInst<Fn>& e : tab)
    if (e.dtype == dtype && e.fa == g.fa && e.fb == g.fb) return e.fn[g.ss];
  return nullptr;
}

// Steps 4 and 5 of mi_gram: launch what the plan says, then finish as it says.
static int gram_launch(const mi_gram_desc* d, const GramPlan& g, void* ws, hipStream_t st) {
  const bool stream = g.family == GRAM_STREAM;
  const GramFn fn = stream ? nullptr : gram_find(GRAM_LDS_TABLE, d->dtype, g);
  const GramSFn sfn = stream ? gram_find(GRAM_STREAM_TABLE, d->dtype, g) : nullptr;
  MI_CHECK_ARG(fn || sfn, "gram: no %s %s kernel with %d x %d fragments%s", stream ? "streaming" : "LDS-staged",
               d->dtype == MI_BF16 ? "bf16" : "fp32", g.fa, g.fb, g.ss ? " and sumsq" : "");
  GramK k;
  k.a = d->a; k.a_bs = d->a_bs; k.a_gs = d->a_gs; k.ma = d->ma;
  k.b = d->b; k.b_bs = d->b_bs; k.b_gs = d->b_gs; k.mb = d->mb;
  k.n = d->n; k.groups = d->groups; k.Z = g.Z; k.fold = g.fold;
  k.chunks_per_split = g.per_split; k.nchunks = g.units; k.tiles_b = g.tiles_b; k.vec_ok = g.vec_ok;
  k.part = g.finish == GRAM_DIRECT ? d->out : (float*)ws;
  k.ss_part = g.ss ? (float*)((char*)ws + g.part_bytes) : nullptr;
  bool deferred = false;
  if (g.deferrable) {
    float* arena = deferred_take(g.part_bytes / sizeof(float), st);
    if (arena) { k.part = arena; deferred = true; }
  }
  const int64_t per = (int64_t)d->ma * d->mb;
  {
    const double ZZ = (double)d->batch * d->groups, es = (double)dtype_size(d->dtype);
    ProfScope ps(st, g.ss ? K_GRAM_QK : K_GRAM, (double)(d->ma + d->mb) * d->n * ZZ * es + 4.0 * g.splits * g.Z * per,
                 2.0 * per * (double)d->n * ZZ);
    if (stream) hipLaunchKernelGGL(sfn, g.grid, g.block, 0, st, k, g.per_split, g.units);
    else hipLaunchKernelGGL(fn, g.grid, g.block, 0, st, k);
  }
  MI_LAUNCH_CHECK();
  if (deferred) {
    MI_TRY(launch_reduce_rows(k.part, d->out, (int64_t)g.splits * g.images, per, per, d->accumulate, 1.0f, st));
  } else if (g.finish != GRAM_DIRECT) {
    ProfScope ps2(st, K_GRAM_REDUCE, 4.0 * (g.splits + 1) * g.Z * per, (double)g.splits * g.Z * per);
    const bool few = g.finish != GRAM_REDUCE;                        // one thread per output element / 16 slice-phases per element
    const auto reduce = g.finish == GRAM_REDUCE_FEW4 ? gram_reduce_few_kernel<4> : (few ? gram_reduce_few_kernel<16> : gram_reduce_kernel);
    hipLaunchKernelGGL(reduce, dim3(cdiv(per, few ? 256 : 16), g.zo), dim3(256), 0, st, (const float*)k.part, d->out,
                       few ? g.total : g.splits, g.images, d->groups, d->ma, d->mb, d->out_ld, d->out_zs, d->sum_batch, d->accumulate);
    MI_LAUNCH_CHECK();
  }
  if (g.ss) {
    const int64_t cols = (int64_t)g.Z * (d->ma + d->mb);
    MI_TRY(launch_reduce_rows(k.ss_part, d->sumsq, g.splits, cols, cols, 0, 1.0f, st));
  }
  return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" size_t mi_gram_workspace(const mi_gram_desc* d) {
  if (!d || d->ma <= 0 || d->mb <= 0 || d->n <= 0 || d->batch <= 0 || d->groups <= 0) return 0;
  // which family runs depends on pointer alignment (and the switches) at call time, and sumsq presence may differ between the
  // sizing call and the real call: cover both families' plans, each with its sumsq rows (GramPlan::ws_bytes)
  return max_of({gram_plan(d, GRAM_LDS).ws_bytes(), gram_plan(d, GRAM_STREAM).ws_bytes()});
}

extern "C" int mi_gram(const mi_gram_desc* d, void* ws, void* stream) {
  MI_TRY(gram_check(d));
  MI_CHECK_ARG(ws, "gram: null workspace");
  const GramPlan g = gram_plan(d);
  MI_CHECK_ARG(g.grid.y <= 65535 && g.grid.z <= 65535, "gram: grid too large");
  return gram_launch(d, g, ws, (hipStream_t)stream);
}

// What mi_gram runs for this descriptor under the current switches.  Host-side only: the same gram_plan, and pointers are read
// for their alignment only (any 16-byte-aligned placeholder will do).  out[22]: family (0 LDS-staged, 1 streaming), fragments
// per tile side fa, fb (32 rows each; streaming: 16), sumsq, contraction unit in pixels, units in total, units per split, splits,
// tiles over A, tiles over B, Z, fold (units per image, 0 = per image), 16-byte rows, grid x / y / z, block, partial bytes, sumsq
// row bytes, finish (0 direct into the output, 1 reduce few<4>, 2 reduce few<16>, 3 general reduce), partials may go to the
// deferred arena, workspace bytes.
extern "C" int mi_gram_plan(const mi_gram_desc* d, int64_t* out) {
  MI_TRY(gram_check(d));
  MI_CHECK_ARG(out, "gram_plan: null pointer");
  const GramPlan g = gram_plan(d);
  const int64_t v[22] = {g.family, g.fa, g.fb, g.ss, g.unit, g.units, g.per_split, g.splits, g.tiles_a, g.tiles_b, g.Z, g.fold, g.vec_ok,
                         g.grid.x, g.grid.y, g.grid.z, g.block.x, (int64_t)g.part_bytes, (int64_t)g.ss_bytes, g.finish, g.deferrable,
                         (int64_t)g.ws_bytes()};
  memcpy(out, v, sizeof(v));
  return MI_OK;
}
