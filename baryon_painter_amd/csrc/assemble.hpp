// Device-side batch assembly: the descriptors of bp_gather_tiles (include/bp_hip.h) and the value of one gathered
// pixel, shared by the plain gather (pointwise.hip) and the gather into a pyramid (scales.hip) so that both store the
// same bits.
#pragma once
#include "common.hpp"
#include <math.h>

// One descriptor per (sample, slab): where the tile starts in the HBM-resident stack and how the
// dihedral tile permutation maps output (r,c) to source (row,col):  row = r0 + rr*r + rc*c, ...
struct TileDesc {
  const float* base;      // &stack[slice][tile_y*t][tile_x*t]
  int32_t pitch;          // n_grid
  int32_t r0, rr, rc, c0, cr, cc;
  int32_t pad_;
};
struct SampleXform {      // x -> log(scale*x * inv_sigma + 1) * inv_k   (mode 1), or scale*x (mode 0)
  double scale, inv_sigma, inv_k;
  int32_t mode, pad_;
};

// float32 sum of the two permuted slab tiles at output (r, c), like the host path's get_stack
__device__ __forceinline__ float tile_sum(const TileDesc& a, const TileDesc& b, int r, int c) {
  const float va = a.base[(int64_t)(a.r0 + a.rr * r + a.rc * c) * a.pitch + (a.c0 + a.cr * r + a.cc * c)];
  const float vb = b.base[(int64_t)(b.r0 + b.rr * r + b.rc * c) * b.pitch + (b.c0 + b.cr * r + b.cc * c)];
  return va + vb;
}

// ... after the SLICS scaling: what the host holds before subtract_minimum and the transform
// (python float * float32 array = a float32 multiply with the scalar rounded to float32, datasets.py:399)
__device__ __forceinline__ float tile_scale(float s, const SampleXform& x) {
  return x.scale == 1.0 ? s : (float)x.scale * s;
}

__device__ __forceinline__ float tile_transform(float s, const SampleXform& x) {
  double v = (double)s;
  if (x.mode == 1) v = log(v * x.inv_sigma + 1.0) * x.inv_k;
  return (float)v;
}
