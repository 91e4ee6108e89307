// bp_gather_tiles_gan: the CGAN's training batch, gathered from the slab stacks in HBM by one launch that writes straight
// into the four places its training plan reads (models/cgan.py, _GanPlan): the generator's input [dm, aux], the real half
// of the discriminator's input [dm, aux, pressure], the conditioning channels [dm, aux] of the fake half, and the dense
// pressure plane of the L1 term.  It stands for two bp_gather_tiles, one host transform per field, an upload, two copies
// and four bp_nchw_to_view launches.
//
// A pixel is bp_gather_tiles' float32 value at mode 0 (assemble.hpp: tile_sum, tile_scale, then the float32 minimum of
// subtract_minimum sets) under the CGAN's "shift-log-cam" transform (range_compress.hpp: rc_shift_log_cam, the function
// bp_paint_load_cam calls): the composition of those two entry points, bit for bit.
//
// Thread map.  A lane owns VP = 4 consecutive pixels of one output row; a workgroup owns 256 such groups of ONE sample, so
// the sample index is a function of blockIdx alone: the four tile descriptors, the two scales, the six transform constants,
// the minimum and aux are wave-uniform loads, fetched once per wave, and the only per-lane division is item / groups.
// Stores are the coalesced side.  The 8 floats [dm, aux] x 4 of gen_in and the 4 floats of x_nchw go out as 16-byte
// stores where the view is dense (cstride 2) and the lane's first byte is 16-byte aligned; the 12-byte pixel of d_real as
// 8 + 4 bytes and the 8-byte pixel of d_fake_cond as 8 bytes where the pixel is 8-byte aligned; 4-byte stores of the same
// values otherwise (odd tiles, channel offsets, row tails).  Bytes between the named channels and cstride are not
// touched: the pad channel of d_in and the fake half's pressure channel belong to others.
// Reads.  Each stack value is read once.  A permutation without transposition reads 16 consecutive bytes per lane (a
// flip: in descending order); a transposing one (rc != 0) reads four rows per lane, strided by the pitch.  No LDS
// transpose: the 128-byte lines such a wave touches are the lines its neighbours in r touch too, and they stay in L2.
// Two double-precision logarithms and four double divisions per pixel: the kernel is bound by those, not by bytes.
#include "common.hpp"
#include "assemble.hpp"
#include "range_compress.hpp"
#include "kernels.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int GB = 256;   // lanes per workgroup
constexpr int VP = 4;     // consecutive pixels of a row per lane

struct GanDst {           // an NHWC destination: pixel p's channels start at p[(int64) pixel * cs + co]
  float* p;
  int cs, co;
};

__device__ __forceinline__ bool aligned_to(const void* p, unsigned bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0u;
}

// [a, b] of `cnt` consecutive pixels
__device__ __forceinline__ void put_pairs(const GanDst& d, int64_t pix, const float (&a)[VP], float b, int cnt) {
  float* o = d.p + pix * d.cs + d.co;
  if (cnt == VP && d.cs == 2 && aligned_to(o, 16)) {
    reinterpret_cast<float4*>(o)[0] = make_float4(a[0], b, a[1], b);
    reinterpret_cast<float4*>(o)[1] = make_float4(a[2], b, a[3], b);
    return;
  }
  const bool two = (d.cs & 1) == 0 && aligned_to(o, 8);      // then every pixel of the lane is 8-byte aligned
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    if (v >= cnt) break;
    float* q = o + (int64_t)v * d.cs;
    if (two) {
      *reinterpret_cast<float2*>(q) = make_float2(a[v], b);
    } else {
      q[0] = a[v];
      q[1] = b;
    }
  }
}

// [a, b, c] of `cnt` consecutive pixels
__device__ __forceinline__ void put_triples(const GanDst& d, int64_t pix, const float (&a)[VP], float b,
                                            const float (&c)[VP], int cnt) {
  float* o = d.p + pix * d.cs + d.co;
  const bool two = (d.cs & 1) == 0 && aligned_to(o, 8);
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    if (v >= cnt) break;
    float* q = o + (int64_t)v * d.cs;
    if (two) {
      *reinterpret_cast<float2*>(q) = make_float2(a[v], b);
    } else {
      q[0] = a[v];
      q[1] = b;
    }
    q[2] = c[v];
  }
}

__device__ __forceinline__ void put_plane(float* x, int64_t pix, const float (&c)[VP], int cnt) {
  float* o = x + pix;
  if (cnt == VP && aligned_to(o, 16)) {
    *reinterpret_cast<float4*>(o) = make_float4(c[0], c[1], c[2], c[3]);
    return;
  }
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    if (v >= cnt) break;
    o[v] = c[v];
  }
}

__global__ __launch_bounds__(GB) void gather_tiles_gan_kernel(const TileDesc* in100, const TileDesc* in150,
                                                              const SampleXform* in_xf, const float* in_minima,
                                                              const TileDesc* lab100, const TileDesc* lab150,
                                                              const SampleXform* lab_xf, const double* cam,
                                                              const float* aux, int t, int groups, int chunks, GanDst gen,
                                                              GanDst real, GanDst fake, float* x) {
  const int n = (int)(blockIdx.x / (unsigned)chunks);                     // wave-uniform: one sample per workgroup
  const int item = (int)(blockIdx.x - (unsigned)n * (unsigned)chunks) * GB + (int)threadIdx.x;
  if (item >= t * groups) return;
  const int r = item / groups, c0 = (item - r * groups) * VP;
  const int cnt = t - c0 < VP ? t - c0 : VP;
  const TileDesc a = in100[n], b = in150[n], la = lab100[n], lb = lab150[n];
  const SampleXform xi = in_xf[n], xl = lab_xf[n];
  const double* cm = cam + (int64_t)n * 6;
  const double si = cm[0], ki0 = cm[1], ki1 = cm[2], sl = cm[3], kl0 = cm[4], kl1 = cm[5];
  const bool sub = in_minima != nullptr;
  const float mn = sub ? in_minima[n] : 0.f;
  const float z = aux[n];
  float dm[VP], pr[VP];
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    const int c = c0 + v < t ? c0 + v : t - 1;                           // (a tail lane re-reads its last pixel: in bounds)
    float s = tile_scale(tile_sum(a, b, r, c), xi);
    if (sub) s = s - mn;
    dm[v] = rc_shift_log_cam(s, si, ki0, ki1);
    pr[v] = rc_shift_log_cam(tile_scale(tile_sum(la, lb, r, c), xl), sl, kl0, kl1);
  }
  const int64_t pix = ((int64_t)n * t + r) * t + c0;
  put_pairs(gen, pix, dm, z, cnt);
  put_triples(real, pix, dm, z, pr, cnt);
  put_pairs(fake, pix, dm, z, cnt);
  put_plane(x, pix, pr, cnt);
}

bool view_is(const bp_view* v, int n, int t, int c) { return v->n == n && v->h == t && v->w == t && v->c == c; }

}  // namespace

int bp_gather_tiles_gan(const void* in100, const void* in150, const void* in_xform, const float* in_minima,
                        const void* lab100, const void* lab150, const void* lab_xform, const double* cam,
                        const float* aux, int32_t n, int32_t tile, const bp_view* gen_in, const bp_view* d_real,
                        const bp_view* d_fake_cond, float* x_nchw, void* stream) {
  if (!in100 || !in150 || !in_xform || !lab100 || !lab150 || !lab_xform || !cam || !aux || !x_nchw || n <= 0 || tile <= 0)
    return BP_EINVAL;
  if (!bp_view_ok_any(gen_in) || !bp_view_ok_any(d_real) || !bp_view_ok_any(d_fake_cond)) return BP_EINVAL;
  if (!view_is(gen_in, n, tile, 2) || !view_is(d_real, n, tile, 3) || !view_is(d_fake_cond, n, tile, 2)) return BP_EINVAL;
  if (gen_in->dtype != BP_F32 || d_real->dtype != BP_F32 || d_fake_cond->dtype != BP_F32) return BP_EUNSUPPORTED;
  if ((int64_t)tile * tile >= (int64_t)1 << 31) return BP_EUNSUPPORTED;
  const int groups = bp_ceil_div(tile, VP);
  const int64_t chunks = ((int64_t)tile * groups + GB - 1) / GB;
  if (chunks * n >= (int64_t)1 << 31) return BP_EUNSUPPORTED;              // (the grid's x extent)
  hipLaunchKernelGGL(gather_tiles_gan_kernel, dim3((unsigned)(chunks * n)), dim3(GB), 0, bp_stream(stream),
                     static_cast<const TileDesc*>(in100), static_cast<const TileDesc*>(in150),
                     static_cast<const SampleXform*>(in_xform), in_minima, static_cast<const TileDesc*>(lab100),
                     static_cast<const TileDesc*>(lab150), static_cast<const SampleXform*>(lab_xform), cam, aux, (int)tile,
                     groups, (int)chunks, GanDst{static_cast<float*>(gen_in->ptr), gen_in->cstride, gen_in->coff},
                     GanDst{static_cast<float*>(d_real->ptr), d_real->cstride, d_real->coff},
                     GanDst{static_cast<float*>(d_fake_cond->ptr), d_fake_cond->cstride, d_fake_cond->coff}, x_nchw);
  BP_CHECK_LAUNCH();
  return BP_OK;
}
