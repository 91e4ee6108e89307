// paint() throughput pipeline (BASELINE.json configs[4], SURVEY.md 8d metric (B), 8f-2): the pieces that sit on
// either side of the captured eval-mode forward so that a RAW dark-matter tile goes in and a physical pressure tile
// comes out without a host-side NumPy pass per tile.
//   bp_paint_load     raw NCHW tile -> shift-log transform (data_transforms.py:76) -> NHWC view + redshift planes
//                     (merge_aux_label, utils.py:159-182): the fused form of the host transform + bp_nchw_to_view
//   bp_paint_store    head view -> [softplus] -> inverse shift-log (data_transforms.py:97) -> NCHW tile: the fused
//                     form of bp_view_to_nchw + the host inverse transform
//   bp_paint_load_mode / bp_paint_load2_mode / bp_paint_store_mode   the same with any of the six range-compression modes
//                     (range_compress.hpp) and records of four float64 per tile; the three above are these at mode
//                     shift-log, reading their two-double tables
//   bp_paint_store_fields   the store of a head with several label fields: per field bp_paint_store_mode's (one level)
//                     or bp_paint_store_scales_mode's (several) expression with the field's own mode and records, in one
//                     launch
//   bp_paint_store_moments  the store of an ensemble: the head holds K latent draws per tile, and the float64 mean and
//                     population variance over the draws of what bp_paint_store_fields would store leave (and, on
//                     request, every draw)
//   bp_paint_load_cam / bp_paint_store_cam   the same pair for the conditional GAN: its "shift-log-cam" transform into the
//                     tanh range, log(x / sigma + 1) / k0 - k1 (painter.CGANPainter.transform), and the generator's tanh
//                     head followed by the inverse, both evaluated in double as the host's NumPy expressions are
//   bp_philox_normal  the prior noise of cvae.py:64-65 from a counter-based generator keyed on (seed, GLOBAL tile id):
//                     a tile's sample does not depend on which batch, stream or rank paints it
//   bp_likelihood_draw  a draw x_mu + sqrt(x_var) e from the likelihood of a two-head CVAE, e from the same generator on
//                     a noise lattice keyed on (seed, noise id, lattice pixel, channel): what the store kernels read
//                     in place of the mean head when a painter paints with pixel noise
// Float semantics are those of the host path (the reference's NumPy expressions on float32 tiles, evaluated in
// double where NumPy promotes to double), so device and host transforms agree to the last float32 bit except for
// libm differences of exp (<= 1 ulp of the exponential).
#include "common.hpp"
#include "range_compress.hpp"
#include <math.h>

namespace {

constexpr int RB = 256;

// (out2: an optional second destination of the same pixels -- the generator reads the transformed tile in its
//  concatenated input as well as the prior network: the double-precision logarithm is taken once, not once per view)
template <int M>
__global__ __launch_bounds__(RB) void paint_load_kernel(const float* src, int c, RcTable xf, const float* aux,
                                                        int caux, float* out, int out_cs, int out_co, float* out2,
                                                        int out2_cs, int out2_co, int64_t hw, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  // (32-bit index arithmetic, shifts where the sizes are powers of two: four 64-bit divisions by run-time values per
  //  element were what this kernel spent its time on -- the entry points check total < 2^31)
  const unsigned ct = (unsigned)(c + caux), iu = (unsigned)i, hwu = (unsigned)hw;
  const unsigned pu = ct == 2u ? iu >> 1 : iu / ct;
  const int ch = (int)(iu - pu * ct);
  const unsigned nu = (hwu & (hwu - 1u)) == 0u ? pu >> (__ffs((int)hwu) - 1) : pu / hwu;
  const int64_t p = pu, n = nu, yx = pu - nu * hwu;
  float v;
  if (ch < c) {
    // e.g. np.log(x / std + 1) / k  with float32 x and float64 std: evaluated in double, stored as float32
    v = rc_forward<M>(rc_record(xf, n), src[(n * c + ch) * hw + yx]);
  } else {
    v = aux[n * caux + (ch - c)];
  }
  out[p * out_cs + out_co + ch] = v;
  if (out2) out2[p * out2_cs + out2_co + ch] = v;
}

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

template <int M>
__global__ __launch_bounds__(RB) void paint_store_kernel(const float* src, int src_cs, int src_co, int c, PW pw,
                                                         int softplus, RcTable xf, float* dst, int64_t hw,
                                                         int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;     // NCHW destination index (coalesced writes)
  if (i >= total) return;
  const unsigned iu = (unsigned)i, hwu = (unsigned)hw;          // (32-bit arithmetic: see paint_load_kernel)
  const unsigned pl = (hwu & (hwu - 1u)) == 0u ? iu >> (__ffs((int)hwu) - 1) : iu / hwu;        // plane = n * c + ch
  const int64_t yx = iu - pl * hwu;
  const unsigned nu = c == 1 ? pl : pl / (unsigned)c;
  const int ch = (int)(pl - nu * (unsigned)c);
  const int64_t n = nu;
  float v = pw_apply(pw, ch, src[(n * hw + yx) * src_cs + src_co + ch]);
  if (softplus) v = softplus_f(v);
  // e.g. (np.exp(x * k) - 1) * std: float32 product, float32 exp, float32 subtraction, double product
  dst[i] = rc_inverse<M>(rc_record(xf, n), v);
}

// Modes of up to FIELDS_MAX label fields, four bits each, as a kernel argument (the entry point's array is the host's)
constexpr int FIELDS_MAX = 64;
constexpr int LEVELS_MAX = 16;
constexpr int DRAWS_MAX = 64;                                   // draws of an ensemble (bp_paint_store_moments)
struct FieldModes {
  unsigned w[FIELDS_MAX / 8];
};

__device__ __forceinline__ float rc_inverse_of(int mode, const RcRec& r, float v) {
  switch (mode) {
    case RC_SHIFT_LOG: return rc_inverse<RC_SHIFT_LOG>(r, v);
    case RC_LOG: return rc_inverse<RC_LOG>(r, v);
    case RC_SHIFT_LOG_2P: return rc_inverse<RC_SHIFT_LOG_2P>(r, v);
    case RC_LOG_TANH: return rc_inverse<RC_LOG_TANH>(r, v);
    case RC_X_1PX: return rc_inverse<RC_X_1PX>(r, v);
    default: return rc_inverse<RC_INV_X>(r, v);
  }
}

// What a field's inverse reads at one pixel: activation and softplus per channel of the field's channels [c0, c0 + used)
// at `s`, then the float32 sum in channel order (used == 1: the channel itself).
__device__ __forceinline__ float field_sum(const float* s, int c0, int used, const PW& pw, int softplus) {
#pragma clang fp contract(off)
  float v = 0.f;
  for (int ch = 0; ch < used; ++ch) {
    float t = pw_apply(pw, c0 + ch, s[c0 + ch]);
    if (softplus) t = softplus_f(t);
    v = ch == 0 ? t : v + t;                                    // ((c0 + c1) + c2) ...: NumPy's order for sum(axis=0)
  }
  return v;
}

// The head of a painter with several label fields: field f owns channels [f * levels, (f + 1) * levels) and plane
// n * fields + f of the (n, fields, H, W) destination.  One thread per PIXEL (n, y, x) of the head, in pixel order: it
// reads the fields * levels contiguous channels of its pixel -- a wave reads whole cache lines, and a head value is
// fetched by one thread of the launch -- and writes one element to each field's plane, so that the lanes of a wave
// write consecutive floats of a plane, field by field (the coalesced NCHW side of paint_store_kernel, its 32-bit index
// arithmetic).  Per field the expression is paint_store_kernel's (levels == 1) or paint_store_scales_kernel's
// (levels > 1) with that field's record.  The field loop is uniform over the wave, so the field's mode -- a run-time
// value of the plane -- is a scalar branch; a workgroup that straddles tiles reads each lane's own records.
__global__ __launch_bounds__(RB) void paint_store_fields_kernel(const float* src, int src_cs, int src_co, int fields,
                                                                int levels, int used, FieldModes modes, PW pw,
                                                                int softplus, const double* records, float* dst,
                                                                unsigned hw, unsigned pixels) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * RB + threadIdx.x;             // pixel n * hw + yx
  if (i >= pixels) return;
  const unsigned nu = (hw & (hw - 1u)) == 0u ? i >> (__ffs((int)hw) - 1) : i / hw;              // (see paint_load_kernel)
  const unsigned yx = i - nu * hw;
  const float* s = src + (int64_t)i * src_cs + src_co;
  for (int f = 0; f < fields; ++f) {
    const float v = field_sum(s, f * levels, used, pw, softplus);
    const int mode = (int)((modes.w[f >> 3] >> ((f & 7) * 4)) & 15u);
    const unsigned pl = nu * (unsigned)fields + (unsigned)f;    // plane of the destination; < n * fields
    dst[(int64_t)pl * hw + yx] = rc_inverse_of(mode, rc_record(rc_table4(records), (int64_t)pl), v);
  }
}

// An ENSEMBLE's store: the head holds draws * n samples, sample l * n + m = draw l of tile m, and what leaves is the
// mean and the population variance over the draws of what paint_store_fields_kernel would store for each sample (p_l,
// with tile m's record), (n, fields, H, W) each, and optionally every p_l, (n, draws, fields, H, W).
//   S = ((p_0 + p_1) + ...) + p_{K-1},  M = S / K,  Q = ((p_0 - M)^2 + (p_1 - M)^2) + ...,  mean = (float) M,
//   var = (float) (Q / K)      in float64, ascending l, no contraction: one thread owns a pixel's draws, no atomics.
// Thread mapping: paint_store_fields_kernel's, over the pixels of the n TILES (V = 1), the draws of a pixel
// `pixels * src_cs` floats apart.  V = 4: four consecutive pixels of a one-channel head with cstride 1 (the entry point
// checks hw % 4 == 0 and the alignment of every pointer), read and written as float4.
// KMAX > 0 (draws <= KMAX): the p_l stay in registers between the two sums.  KMAX == 0: a second pass reads and
// evaluates them again -- the same instructions on the same values, hence the same bits.
template <int V>
__device__ __forceinline__ void moments_draw(const float* s, int c0, int used, const PW& pw, int softplus, int mode,
                                             const RcRec& rec, float (&p)[V]) {
#pragma clang fp contract(off)
  if (V == 1) {
    p[0] = rc_inverse_of(mode, rec, field_sum(s, c0, used, pw, softplus));
  } else {                                                      // (one field of one channel, c0 == 0)
    const float4 q = *reinterpret_cast<const float4*>(s);
    const float t[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float x = pw_apply(pw, 0, t[v]);
      if (softplus) x = softplus_f(x);
      p[v] = rc_inverse_of(mode, rec, x);
    }
  }
}

template <int V>
__device__ __forceinline__ void moments_put(float* dst, const float (&p)[V]) {
  if (V == 1) *dst = p[0];
  else *reinterpret_cast<float4*>(dst) = make_float4(p[0], p[1], p[2], p[3]);
}

template <int KMAX, int V>
__global__ __launch_bounds__(RB) void paint_store_moments_kernel(const float* src, int src_cs, int src_co, int fields,
                                                                 int levels, int used, FieldModes modes, PW pw,
                                                                 int softplus, const double* records, int draws,
                                                                 float* mean, float* var, float* out, unsigned hw,
                                                                 unsigned pixels) {
#pragma clang fp contract(off)
  const unsigned i = (blockIdx.x * RB + threadIdx.x) * V;       // first pixel m * hw + yx of this thread
  if (i >= pixels) return;
  const unsigned nu = (hw & (hw - 1u)) == 0u ? i >> (__ffs((int)hw) - 1) : i / hw;              // (see paint_load_kernel)
  const unsigned yx = i - nu * hw;
  const int64_t lstride = (int64_t)pixels * src_cs;             // floats between two draws of a pixel
  const float* s0 = src + (int64_t)i * src_cs + src_co;
  const double K = (double)draws;
  for (int f = 0; f < fields; ++f) {
    const int c0 = f * levels;
    const int mode = (int)((modes.w[f >> 3] >> ((f & 7) * 4)) & 15u);
    const unsigned pl = nu * (unsigned)fields + (unsigned)f;    // plane of mean / var; < n * fields
    const RcRec rec = rc_record(rc_table4(records), (int64_t)pl);
    // plane (m, l, f) of the draws: ((m * K + l) * fields + f) * hw + yx
    float* o = out ? out + ((int64_t)nu * draws * fields + f) * hw + yx : nullptr;
    const int64_t ostride = (int64_t)fields * hw;
    double S[V], Q[V], M[V];
    if constexpr (KMAX > 0) {
      float p[KMAX][V];
#pragma unroll
      for (int l = 0; l < KMAX; ++l) {
        if (l < draws) {
          moments_draw<V>(s0 + l * lstride, c0, used, pw, softplus, mode, rec, p[l]);
          if (o) moments_put<V>(o + l * ostride, p[l]);
#pragma unroll
          for (int v = 0; v < V; ++v) S[v] = l == 0 ? (double)p[l][v] : S[v] + (double)p[l][v];
        }
      }
#pragma unroll
      for (int v = 0; v < V; ++v) M[v] = S[v] / K;
#pragma unroll
      for (int l = 0; l < KMAX; ++l) {
        if (l < draws) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const double d = (double)p[l][v] - M[v];
            Q[v] = l == 0 ? d * d : Q[v] + d * d;
          }
        }
      }
    } else {
      float p[V];
      for (int l = 0; l < draws; ++l) {
        moments_draw<V>(s0 + l * lstride, c0, used, pw, softplus, mode, rec, p);
        if (o) moments_put<V>(o + l * ostride, p);
#pragma unroll
        for (int v = 0; v < V; ++v) S[v] = l == 0 ? (double)p[v] : S[v] + (double)p[v];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) M[v] = S[v] / K;
      for (int l = 0; l < draws; ++l) {
        moments_draw<V>(s0 + l * lstride, c0, used, pw, softplus, mode, rec, p);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double d = (double)p[v] - M[v];
          Q[v] = l == 0 ? d * d : Q[v] + d * d;
        }
      }
    }
    float mo[V], vo[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      mo[v] = (float)M[v];
      vo[v] = (float)(Q[v] / K);
    }
    moments_put<V>(mean + (int64_t)pl * hw + yx, mo);
    moments_put<V>(var + (int64_t)pl * hw + yx, vo);
  }
}

// The CGAN's pair.  Same thread-to-element maps as the two kernels above (NHWC order on the way in, NCHW order on the
// way out: the side that is written is the coalesced one), same 32-bit index arithmetic.  xf holds three doubles per
// sample: {sigma, k0, k1} on the way in, {k0, k1, sigma} on the way out.
__global__ __launch_bounds__(RB) void paint_load_cam_kernel(const float* src, int c, const double* xf, const float* aux,
                                                            int caux, float* out, int out_cs, int out_co, int64_t hw,
                                                            int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i >= total) return;
  const unsigned ct = (unsigned)(c + caux), iu = (unsigned)i, hwu = (unsigned)hw;
  const unsigned pu = ct == 2u ? iu >> 1 : iu / ct;
  const int ch = (int)(iu - pu * ct);
  const unsigned nu = (hwu & (hwu - 1u)) == 0u ? pu >> (__ffs((int)hwu) - 1) : pu / hwu;
  const int64_t p = pu, n = nu, yx = pu - nu * hwu;
  float v;
  if (ch < c) {
    // np.log(x / sigma + 1) / k0 - k1 with float32 x and float64 sigma: evaluated in double, stored as float32
    v = rc_shift_log_cam(src[(n * c + ch) * hw + yx], xf[3 * n], xf[3 * n + 1], xf[3 * n + 2]);
  } else {
    v = aux[n * caux + (ch - c)];
  }
  out[p * out_cs + out_co + ch] = v;
}

__global__ __launch_bounds__(RB) void paint_store_cam_kernel(const float* src, int src_cs, int src_co, int c,
                                                             const double* xf, float* dst, int64_t hw, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;     // NCHW destination index (coalesced writes)
  if (i >= total) return;
  const unsigned iu = (unsigned)i, hwu = (unsigned)hw;
  const unsigned pl = (hwu & (hwu - 1u)) == 0u ? iu >> (__ffs((int)hwu) - 1) : iu / hwu;        // plane = n * c + ch
  const int64_t yx = iu - pl * hwu;
  const unsigned nu = c == 1 ? pl : pl / (unsigned)c;
  const int ch = (int)(pl - nu * (unsigned)c);
  const int64_t n = nu;
  // the generator's head: the float32 tanh of bp_unary_forward; then (np.exp((y + k1) * k0) - 1) * sigma in double
  const double y = (double)tanhf(src[(n * hw + yx) * src_cs + src_co + ch]);
  dst[i] = (float)((exp((y + xf[3 * n + 1]) * xf[3 * n]) - 1.0) * xf[3 * n + 2]);
}

// Philox4x32-10 (Salmon et al. 2011): counter (c0..c3), key (k0, k1)
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
  const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
  c[0] = h1 ^ c[1] ^ k0; c[1] = l1; c[2] = h0 ^ c[3] ^ k1; c[3] = l0;
}

// eps[(l * n + s) * per_tile + i], i = 4 * g + r: r-th normal of Philox block (g, l, tile id) under key = seed.
// Box-Muller in double on the uniforms u1 = (x + 1) / 2^32 in (0, 1], u2 = x / 2^32 in [0, 1).
// (seed_dev != nullptr: the key is read from device memory, so that a captured graph serves every seed)
__global__ __launch_bounds__(RB) void philox_normal_kernel(unsigned long long seed, const unsigned long long* seed_dev,
                                                           const long long* tile_ids, int n, int L, int per_tile,
                                                           float* eps) {
  if (seed_dev) seed = *seed_dev;
  const int groups = (per_tile + 3) / 4;
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i >= (int64_t)L * n * groups) return;
  const int g = i % groups;
  const int s = (i / groups) % n;
  const int l = i / ((int64_t)groups * n);
  const unsigned long long tid = (unsigned long long)tile_ids[s];
  unsigned c[4] = {(unsigned)g, (unsigned)l, (unsigned)tid, (unsigned)(tid >> 32)};
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const double two32 = 4294967296.0, twopi = 6.283185307179586476925286766559;
  double z[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double u1 = ((double)c[2 * h] + 1.0) / two32, u2 = (double)c[2 * h + 1] / two32;
    const double rad = sqrt(-2.0 * log(u1));
    z[2 * h] = rad * cos(twopi * u2);
    z[2 * h + 1] = rad * sin(twopi * u2);
  }
  float* o = eps + ((int64_t)l * n + s) * per_tile + 4 * g;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * g + r < per_tile) o[r] = (float)z[r];
}

// A draw from the likelihood, out = t + sqrt(var) e: t the mean head (softplus as in paint_store_kernel), var the
// exponential of the variance head, e a pixel of a NOISE LATTICE -- the r-th normal (philox_normal_kernel's Box-Muller,
// in double) of the Philox block with the counter (X + ((ch / 4) << 24), 2^31 | Y, id), r = ch % 4, (Y, X) = the
// sample's origin + (y, x).  Bit 31 of word 1 keeps these blocks apart from the latent draws (l < 2^31) under one key.
// One thread per Philox block = one pixel and one group of four channels, in pixel order: the lanes of a wave read and
// write the (up to four) consecutive channels of consecutive pixels.  Only the half-blocks whose normals the group
// uses go through the double-precision logarithm and sine / cosine (one channel: one logarithm and one cosine).
// Contraction is off: the product and the sum each round once, as the host's float32 restatement does.  A zero product
// (var = 0) leaves t as it is, the sign of a zero and a NaN's payload included.
__global__ __launch_bounds__(RB) void likelihood_draw_kernel(const float* mu, int mu_cs, int mu_co, int softplus,
                                                             const float* lv, int lv_cs, int lv_co,
                                                             const unsigned long long* seed_dev, const long long* ids,
                                                             const int* origins, float* out, int out_cs, int out_co,
                                                             int c, unsigned groups, unsigned w, unsigned hw,
                                                             unsigned total) {
#pragma clang fp contract(off)
  const unsigned i = blockIdx.x * RB + threadIdx.x;             // pixel * groups + g
  if (i >= total) return;
  const unsigned p = groups == 1u ? i : i / groups;             // pixel n * hw + yx
  const unsigned g = i - p * groups;
  const unsigned nu = (hw & (hw - 1u)) == 0u ? p >> (__ffs((int)hw) - 1) : p / hw;              // (see paint_load_kernel)
  const unsigned yx = p - nu * hw;
  const unsigned y = yx / w, x = yx - y * w;
  const unsigned oy = origins ? (unsigned)origins[2 * nu] : 0u, ox = origins ? (unsigned)origins[2 * nu + 1] : 0u;
  const unsigned long long seed = *seed_dev, id = (unsigned long long)ids[nu];
  unsigned ctr[4] = {(ox + x) + (g << 24), 0x80000000u | (oy + y), (unsigned)id, (unsigned)(id >> 32)};
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(ctr, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const int cnt = min(4, c - 4 * (int)g);                       // channels of this group: uniform over the wave if c <= 4
  const double two32 = 4294967296.0, twopi = 6.283185307179586476925286766559;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (2 * h < cnt) {
      const double u1 = ((double)ctr[2 * h] + 1.0) / two32, u2 = (double)ctr[2 * h + 1] / two32;
      const double rad = sqrt(-2.0 * log(u1));
      z[2 * h] = rad * cos(twopi * u2);
      if (2 * h + 1 < cnt) z[2 * h + 1] = rad * sin(twopi * u2);
    }
  }
  const float* m = mu + (int64_t)p * mu_cs + mu_co + 4 * g;
  const float* v = lv + (int64_t)p * lv_cs + lv_co + 4 * g;
  float* o = out + (int64_t)p * out_cs + out_co + 4 * g;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r < cnt) {
      float t = m[r];
      if (softplus) t = softplus_f(t);
      const float s = expf(0.5f * v[r]) * (float)z[r];
      o[r] = s == 0.f ? t : t + s;
    }
  }
}

static inline unsigned nblocks(int64_t total) { return (unsigned)((total + RB - 1) / RB); }

template <int V>
static void launch_moments(int kmax, unsigned blocks, hipStream_t st, const bp_view* src, int fields, int levels, int used,
                           const FieldModes& fm, PW pw, int softplus, const double* records, int draws, float* mean,
                           float* var, float* out, unsigned hw, unsigned pixels) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RB), 0, st, src->ptr, src->cstride, src->coff, fields, levels, used, fm,
                       pw, softplus, records, draws, mean, var, out, hw, pixels);
  };
  if (kmax == 4) go(paint_store_moments_kernel<4, V>);
  else if (kmax == 16) go(paint_store_moments_kernel<16, V>);
  else go(paint_store_moments_kernel<0, V>);
}

}  // namespace

extern "C" {

// out2 == nullptr: one destination
static int paint_load_any(int32_t mode, const float* raw_nchw, int32_t c, RcTable xf, const float* aux, int32_t caux,
                          const bp_view* out, const bp_view* out2, void* stream) {
  if (mode < 0 || mode >= RC_MODES) return BP_EINVAL;
  if (!raw_nchw || !xf.p || !bp_view_ok_any(out) || (out2 && !bp_view_ok_any(out2)) || c <= 0 || caux < 0 ||
      out->c != c + caux || (caux > 0 && !aux))
    return BP_EINVAL;
  if (out2 && (out2->c != out->c || out2->n != out->n || out2->h != out->h || out2->w != out->w)) return BP_EINVAL;
  if (out->dtype != BP_F32 || (out2 && out2->dtype != BP_F32)) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)out->h * out->w, total = (int64_t)out->n * hw * (c + caux);
  if (total >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  rc_dispatch(mode, [&](auto m) {
    paint_load_kernel<decltype(m)::value><<<dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream)>>>(
        raw_nchw, c, xf, aux, caux, out->ptr, out->cstride, out->coff, out2 ? out2->ptr : (float*)nullptr,
        out2 ? out2->cstride : 0, out2 ? out2->coff : 0, hw, total);
  });
  BP_CHECK_LAUNCH();
  return BP_OK;
}

static int paint_store_any(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus, RcTable xf,
                           float* dst_nchw, void* stream) {
  if (mode < 0 || mode >= RC_MODES) return BP_EINVAL;
  if (!bp_view_ok_any(src) || !xf.p || !dst_nchw) return BP_EINVAL;
  if (src->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)src->h * src->w, total = (int64_t)src->n * hw * src->c;
  if (total >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  rc_dispatch(mode, [&](auto m) {
    paint_store_kernel<decltype(m)::value><<<dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream)>>>(
        src->ptr, src->cstride, src->coff, src->c, bp_pw(pw), softplus, xf, dst_nchw, hw, total);
  });
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_paint_load_mode(int32_t mode, const float* raw_nchw, int32_t c, const double* records, const float* aux,
                       int32_t caux, const bp_view* out, void* stream) {
  return paint_load_any(mode, raw_nchw, c, rc_table4(records), aux, caux, out, nullptr, stream);
}

int bp_paint_load2_mode(int32_t mode, const float* raw_nchw, int32_t c, const double* records, const float* aux,
                        int32_t caux, const bp_view* out, const bp_view* out2, void* stream) {
  if (!out2) return BP_EINVAL;
  return paint_load_any(mode, raw_nchw, c, rc_table4(records), aux, caux, out, out2, stream);
}

int bp_paint_store_mode(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* records,
                        float* dst_nchw, void* stream) {
  return paint_store_any(mode, src, pw, softplus, rc_table4(records), dst_nchw, stream);
}

int bp_paint_store_fields(const int32_t* modes, int32_t fields, int32_t levels, int32_t include_original,
                          const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* records,
                          float* dst_nchw, void* stream) {
  if (!modes || !bp_view_ok_any(src) || !records || !dst_nchw) return BP_EINVAL;
  if (fields < 1 || levels < 1 || (int64_t)fields * levels != src->c) return BP_EINVAL;
  for (int f = 0; f < fields; ++f)
    if (modes[f] < 0 || modes[f] >= RC_MODES) return BP_EINVAL;
  if (src->dtype != BP_F32 || levels > LEVELS_MAX || fields > FIELDS_MAX) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)src->h * src->w, pixels = (int64_t)src->n * hw;
  if (pixels * src->c >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  FieldModes fm{};
  for (int f = 0; f < fields; ++f) fm.w[f >> 3] |= (unsigned)modes[f] << ((f & 7) * 4);
  const int used = include_original && levels > 1 ? 1 : levels;       // (one level: the channel itself either way)
  hipLaunchKernelGGL(paint_store_fields_kernel, dim3(nblocks(pixels)), dim3(RB), 0, bp_stream(stream), src->ptr,
                     src->cstride, src->coff, (int)fields, (int)levels, used, fm, bp_pw(pw), softplus ? 1 : 0, records,
                     dst_nchw, (unsigned)hw, (unsigned)pixels);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_paint_store_moments(const int32_t* modes, int32_t fields, int32_t levels, int32_t include_original,
                           const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* records,
                           int32_t draws, float* mean_nchw, float* var_nchw, float* draws_nchw, void* stream) {
  if (!modes || !bp_view_ok_any(src) || !records || !mean_nchw || !var_nchw) return BP_EINVAL;
  if (fields < 1 || levels < 1 || draws < 1 || (int64_t)fields * levels != src->c || src->n % draws != 0) return BP_EINVAL;
  for (int f = 0; f < fields; ++f)
    if (modes[f] < 0 || modes[f] >= RC_MODES) return BP_EINVAL;
  if (src->dtype != BP_F32 || draws > DRAWS_MAX || levels > LEVELS_MAX || fields > FIELDS_MAX) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)src->h * src->w, pixels = (int64_t)(src->n / draws) * hw;
  if (pixels * draws * src->c >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  FieldModes fm{};
  for (int f = 0; f < fields; ++f) fm.w[f >> 3] |= (unsigned)modes[f] << ((f & 7) * 4);
  const int used = include_original && levels > 1 ? 1 : levels;       // (one level: the channel itself either way)
  const int kmax = draws <= 4 ? 4 : draws <= 16 ? 16 : 0;             // draws kept in registers, or two passes
  auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  // 16-byte accesses: a one-channel head with cstride 1 (NHWC and NCHW are the same bytes) whose planes are multiples
  // of four pixels
  const bool v4 = src->c == 1 && src->cstride == 1 && hw % 4 == 0 && aligned(src->ptr) && aligned(mean_nchw) &&
                  aligned(var_nchw) && aligned(draws_nchw);
  if (v4)
    launch_moments<4>(kmax, nblocks(pixels / 4), bp_stream(stream), src, fields, levels, used, fm, bp_pw(pw),
                      softplus ? 1 : 0, records, draws, mean_nchw, var_nchw, draws_nchw, (unsigned)hw, (unsigned)pixels);
  else
    launch_moments<1>(kmax, nblocks(pixels), bp_stream(stream), src, fields, levels, used, fm, bp_pw(pw),
                      softplus ? 1 : 0, records, draws, mean_nchw, var_nchw, draws_nchw, (unsigned)hw, (unsigned)pixels);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

// The shift-log forms: the same kernels at RC_SHIFT_LOG over the tables of two doubles, {sigma, k} / {k, sigma}
// (a bf16 view is BP_EINVAL here, as it has always been).
int bp_paint_load(const float* raw_nchw, int32_t c, const double* sigma_k, const float* aux, int32_t caux,
                  const bp_view* out, void* stream) {
  if (!bp_view_ok(out)) return BP_EINVAL;
  return paint_load_any(RC_SHIFT_LOG, raw_nchw, c, RcTable{sigma_k, 2, 0, 1}, aux, caux, out, nullptr, stream);
}

int bp_paint_load2(const float* raw_nchw, int32_t c, const double* sigma_k, const float* aux, int32_t caux,
                   const bp_view* out, const bp_view* out2, void* stream) {
  if (!bp_view_ok(out) || !bp_view_ok(out2)) return BP_EINVAL;
  return paint_load_any(RC_SHIFT_LOG, raw_nchw, c, RcTable{sigma_k, 2, 0, 1}, aux, caux, out, out2, stream);
}

int bp_paint_store(const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* k_sigma, float* dst_nchw,
                   void* stream) {
  if (!bp_view_ok(src)) return BP_EINVAL;
  return paint_store_any(RC_SHIFT_LOG, src, pw, softplus, RcTable{k_sigma, 2, 1, 0}, dst_nchw, stream);
}

// A bf16 view is a well-formed view these two have no form for (the CGAN has no bf16 mode): BP_EUNSUPPORTED.
int bp_paint_load_cam(const float* raw_nchw, int32_t c, const double* xf, const float* aux, int32_t caux,
                      const bp_view* out, void* stream) {
  if (!raw_nchw || !xf || !bp_view_ok_any(out) || c <= 0 || caux < 0 || out->c != c + caux || (caux > 0 && !aux))
    return BP_EINVAL;
  if (out->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)out->h * out->w, total = (int64_t)out->n * hw * (c + caux);
  if (total >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  hipLaunchKernelGGL(paint_load_cam_kernel, dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream), raw_nchw, c, xf, aux,
                     caux, out->ptr, out->cstride, out->coff, hw, total);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_paint_store_cam(const bp_view* src, const double* xf, float* dst_nchw, void* stream) {
  if (!bp_view_ok_any(src) || !xf || !dst_nchw) return BP_EINVAL;
  if (src->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)src->h * src->w, total = (int64_t)src->n * hw * src->c;
  if (total >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  hipLaunchKernelGGL(paint_store_cam_kernel, dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream), src->ptr,
                     src->cstride, src->coff, src->c, xf, dst_nchw, hw, total);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_philox_normal(uint64_t seed, const int64_t* tile_ids, int32_t n, int32_t L, int32_t per_tile, float* eps,
                     void* stream) {
  if (!tile_ids || n <= 0 || L <= 0 || per_tile <= 0 || !eps) return BP_EINVAL;
  const int64_t total = (int64_t)L * n * ((per_tile + 3) / 4);
  hipLaunchKernelGGL(philox_normal_kernel, dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream),
                     (unsigned long long)seed, (const unsigned long long*)nullptr,
                     reinterpret_cast<const long long*>(tile_ids), n, L, per_tile, eps);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_philox_normal_dev(const uint64_t* seed_dev, const int64_t* tile_ids, int32_t n, int32_t L, int32_t per_tile,
                         float* eps, void* stream) {
  if (!seed_dev || !tile_ids || n <= 0 || L <= 0 || per_tile <= 0 || !eps) return BP_EINVAL;
  const int64_t total = (int64_t)L * n * ((per_tile + 3) / 4);
  hipLaunchKernelGGL(philox_normal_kernel, dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream), 0ull,
                     reinterpret_cast<const unsigned long long*>(seed_dev),
                     reinterpret_cast<const long long*>(tile_ids), n, L, per_tile, eps);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

int bp_likelihood_draw(const bp_view* mu, int32_t softplus, const bp_view* log_var, const uint64_t* seed_dev,
                       const int64_t* noise_ids, const int32_t* origins, const bp_view* out, void* stream) {
  if (!bp_view_ok_any(mu) || !bp_view_ok_any(log_var) || !bp_view_ok_any(out) || !seed_dev || !noise_ids)
    return BP_EINVAL;
  for (const bp_view* v : {log_var, out})
    if (v->n != mu->n || v->h != mu->h || v->w != mu->w || v->c != mu->c) return BP_EINVAL;
  if (mu->dtype != BP_F32 || log_var->dtype != BP_F32 || out->dtype != BP_F32) return BP_EUNSUPPORTED;
  const int64_t hw = (int64_t)mu->h * mu->w, pixels = (int64_t)mu->n * hw;
  if (pixels * mu->c >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  const int64_t groups = (mu->c + 3) / 4, total = pixels * groups;      // <= pixels * c < 2^31
  hipLaunchKernelGGL(likelihood_draw_kernel, dim3(nblocks(total)), dim3(RB), 0, bp_stream(stream), mu->ptr, mu->cstride,
                     mu->coff, softplus ? 1 : 0, log_var->ptr, log_var->cstride, log_var->coff,
                     reinterpret_cast<const unsigned long long*>(seed_dev), reinterpret_cast<const long long*>(noise_ids),
                     origins, out->ptr, out->cstride, out->coff, (int)mu->c, (unsigned)groups, (unsigned)mu->w,
                     (unsigned)hw, (unsigned)total);
  BP_CHECK_LAUNCH();
  return BP_OK;
}

}  // extern "C"
