// Compton-y map of a light cone on the device (lightcone.project_planes(on_device=True), process_SLICS.py:55-64): a
// painted float64 plane P (n x n) is added into the y map (res x res) as
//   y += scipy.ndimage.zoom(where(isnan(P), 0, P) * s, res / n, order=ORDER, mode="mirror")
// in float64 for ORDER 2 ... 5.  The prefilter and the sampler are spline_ws.hpp's (the chunked, parallel prefilter
// under whole-sample symmetric boundaries; bp_plane_cut's zoom is the half-sample "reflect" one, and a thread per line;
// this file is neither).  What is this file's own: NaN -> 0 and the scale are applied where the first pass loads P, and
// the sampler adds into y.  No atomics anywhere: the same inputs give the same bits.  Compiled without floating-point
// contraction, like plane.hip.
#include "spline_ws.hpp"

#pragma clang fp contract(off)

namespace {

// the first pass's load: P itself, NaN -> 0, times `scale`
struct PlaneLoad {
  const double* plane;
  int n;
  double scale;
  __device__ __forceinline__ double operator()(int r, int c) const {
    double v = plane[(size_t)r * n + c];
    if (isnan(v)) v = 0.0;
    v *= scale;
    return v;
  }
};

// the sampler's store: y += v, each pixel read and written once
struct AddStore {
  double* y;
  __device__ __forceinline__ void operator()(unsigned o, double v) const { y[o] += v; }
};

// the three launches of one plane at one order (arguments checked by the caller)
template <int ORDER>
void project_launch(const double* plane, int n, double scale, double* scratch, double* y, int res, hipStream_t sm) {
  spline_zoom_launch<ORDER>(PlaneLoad{plane, n, scale}, n, scratch, AddStore{y}, res, sm);
}

}  // namespace

extern "C" {

size_t bp_plane_project_order_workspace(int32_t n, int32_t res, int32_t order) {
  if (n < 2 || res < 2 || order < 2 || order > 5) return 0;
  return (size_t)2 * n * n * sizeof(double);
}

int bp_plane_project_order(const double* plane, int32_t rows, int32_t cols, double scale, int32_t order,
                           double* scratch, size_t scratch_bytes, double* y, int32_t res, void* stream) {
  if (!plane || !scratch || !y || rows != cols || rows < 2 || res < 2) return BP_EINVAL;
  if (order < 2 || order > 5) return BP_EUNSUPPORTED;
  const int n = rows;
  if ((int64_t)n * n >= ((int64_t)1 << 31) || (int64_t)res * res >= ((int64_t)1 << 31)) return BP_EUNSUPPORTED;
  if (scratch_bytes < bp_plane_project_order_workspace(n, res, order)) return BP_EWORKSPACE;
  const hipStream_t sm = bp_stream(stream);
  switch (order) {
    case 2: project_launch<2>(plane, n, scale, scratch, y, res, sm); break;
    case 3: project_launch<3>(plane, n, scale, scratch, y, res, sm); break;
    case 4: project_launch<4>(plane, n, scale, scratch, y, res, sm); break;
    default: project_launch<5>(plane, n, scale, scratch, y, res, sm); break;
  }
  BP_CHECK_LAUNCH();
  return BP_OK;
}

size_t bp_plane_project_workspace(int32_t n, int32_t res) { return bp_plane_project_order_workspace(n, res, 3); }

int bp_plane_project(const double* plane, int32_t rows, int32_t cols, double scale, double* scratch,
                     size_t scratch_bytes, double* y, int32_t res, void* stream) {
  return bp_plane_project_order(plane, rows, cols, scale, 3, scratch, scratch_bytes, y, res, stream);
}

}  // extern "C"
