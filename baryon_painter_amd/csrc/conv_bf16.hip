// bf16 matrix-core convolutions: configuration, weight packing and the entry points behind capi.hip
// (kernels: conv_bf16.hpp, instantiated per channel-chunk width in conv_bf16_cc*.hip).
#include "conv_bf16.hpp"

using namespace bpbf16;

namespace {

struct BPackArgs {
  const float* w; u16* dst;
  int64_t sa, sb;
  int k, stride, pad, tapsy, nphase, transposed, IS;
  int cin_g, cout_g, CC, nchunk, cout_padP, COB, NT, nrun;
  int run_xm[16], run_xq[16];
  int64_t total;
};

__global__ __launch_bounds__(256) void pack_bf16_kernel(BPackArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  int64_t r = i;
  const int k8 = r % 8; r /= 8;
  const int row = r % a.COB; r /= a.COB;
  const int kq = r % 4; r /= 4;
  const int cb = r % (a.cout_padP / a.COB); r /= (a.cout_padP / a.COB);
  const int kk = kq * 8 + k8;
  const int jb_abs = cb * a.COB + row;
  const int chunk = r % a.nchunk; r /= a.nchunk;
  const int s = r % a.nrun; r /= a.nrun;
  const int ty = r % a.tapsy; r /= a.tapsy;
  const int ph = (int)r;
  const int py = ph / a.nphase, px = ph % a.nphase;
  const int blk = jb_abs / a.COB, jb = jb_abs % a.COB;
  const int co = blk * a.COB + b_channel_of(a.NT, jb);
  const int j = kk / a.CC, cc = kk % a.CC;
  const int tx = a.run_xm[s] + a.IS * (a.run_xq[s] + j);
  const int ci = chunk * a.CC + cc;
  int ky, kx;
  if (a.transposed) {
    ky = bp_t_ky(py, a.pad, a.stride, a.tapsy, ty);
    kx = tx < a.tapsy ? bp_t_ky(px, a.pad, a.stride, a.tapsy, tx) : -1;
  } else {
    ky = ty; kx = tx < a.tapsy ? tx : -1;
  }
  float v = 0.f;
  if (ci < a.cin_g && co < a.cout_g && ky < a.k && kx >= 0 && kx < a.k) v = a.w[ci * a.sa + co * a.sb + ky * a.k + kx];
  a.dst[i] = f2bf(v);
}

}  // namespace

// ---- entry points used by capi.hip
bool bp_bf16_igemm_ok(const ConvGeom& g, const bp_view* in, const bp_view* out) {
  const BConfig c = b_config(g);
  if (!c.ok) return false;
  if (in) {
    const int U = c.CC < 8 ? c.CC : 8;
    const int esz = in->dtype == BP_BF16 ? 2 : 4;
    const int bytes = U * esz < 16 ? U * esz : 16;        // widest single load of a unit
    if ((in->cstride * esz) % bytes || (in->coff * esz) % bytes || reinterpret_cast<uintptr_t>(in->ptr) % 16) return false;
    if (in->c != g.cin_g && !(c.CC == 4 && in->coff + 4 <= in->cstride)) return false;
  }
  if (out && out->dtype == BP_BF16) {
    const int need = c.NT == 1 ? 4 : 8;
    if (out->cstride % need || out->coff % need || reinterpret_cast<uintptr_t>(out->ptr) % 16) return false;
  }
  return true;
}

// The packed image: [generic | flattened-K (conv_bf16_flat.hip) | weights-stationary (conv_bf16_ws.hip) | head
// (conv_bf16_head.hip)], the last three where those kernels apply.  Offsets in elements; the generic image starts at 0
// and ends where the flattened-K one starts.
struct BLayout { int64_t generic, flat, ws, head, total; };
static BLayout bf16_layout(const ConvGeom& g, const BConfig& c) {
  BLayout l;
  l.generic = 0;
  l.flat = (int64_t)g.nphase * g.nphase * g.taps * c.nrun * c.nchunk * c.cout_padP * 32;
  l.ws = l.flat + bp_bf16_flat_packed_elems(g);
  l.head = l.ws + bp_bf16_ws_packed_elems(g);
  l.total = l.head + bp_bf16_head_packed_elems(g);
  return l;
}

int64_t bp_bf16_packed_elems(const ConvGeom& g) {
  const BConfig c = b_config(g);
  return c.ok ? bf16_layout(g, c).total : -1;
}

int bp_bf16_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, void* packed, hipStream_t st) {
  const BConfig c = b_config(g);
  if (!c.ok) return BP_EUNSUPPORTED;
  BPackArgs a{};
  a.w = w_torch; a.dst = reinterpret_cast<u16*>(packed); a.sa = wm.sa; a.sb = wm.sb;
  a.k = g.k; a.stride = g.stride; a.pad = g.pad; a.tapsy = g.taps; a.nphase = g.nphase;
  a.transposed = g.gather_transposed; a.IS = g.IS; a.cin_g = g.cin_g; a.cout_g = g.cout_g;
  a.CC = c.CC; a.nchunk = c.nchunk; a.cout_padP = c.cout_padP; a.COB = c.COB; a.NT = c.NT; a.nrun = c.nrun;
  for (int s = 0; s < c.nrun; ++s) { a.run_xm[s] = c.run_xm[s]; a.run_xq[s] = c.run_xq[s]; }
  const BLayout l = bf16_layout(g, c);
  a.total = l.flat;
  hipLaunchKernelGGL(pack_bf16_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
  BP_CHECK_LAUNCH();
  int rc = BP_OK;
  if (l.ws > l.flat) rc = bp_bf16_flat_pack(g, wm, w_torch, a.dst + l.flat, st);
  if (rc == BP_OK && l.head > l.ws) rc = bp_bf16_ws_pack(g, wm, w_torch, a.dst + l.ws, st);
  if (rc == BP_OK && l.total > l.head) rc = bp_bf16_head_pack(g, wm, w_torch, a.dst + l.head, st);
  return rc;
}

// The order in which the kernels are offered a layer.  bp_bf16_stats_workspace and bp_bf16_igemm_run both walk it; what
// each asks of a kernel differs (the run takes the head kernel only without a pending activation, the workspace asks it
// in mode 3 only), so each walk keeps its own guards: every case holds what belongs to that kernel alone, and the one
// gate that is not a kernel's own -- all but the head kernel need views that bp_bf16_igemm_ok accepts -- stands in front
// of the switch.
enum BKernel { B_HEAD, B_FLAT, B_WS, B_GENERIC };
static const BKernel B_ORDER[] = {B_HEAD, B_FLAT, B_WS, B_GENERIC};

static int64_t bf16_stat_rows(const ConvGeom& g, const BConfig& c, const bp_view* in, const bp_view* out) {
  const int qh = bp_ceil_div(out->h, g.OS), qw = bp_ceil_div(out->w, g.OS);
  return (int64_t)bp_ceil_div(qw, 16 * c.TPR) * bp_ceil_div(qh, c.BH) * in->n * g.nphase * g.nphase;
}

// workspace for bp_bf16_igemm_run with statistics (0: not available for this layer / these views)
size_t bp_bf16_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode) {
  const BConfig c = b_config(g);
  if (!c.ok) return 0;
  const bool views_ok = bp_bf16_igemm_ok(g, in, out);
  for (const BKernel k : B_ORDER) {
    if (k != B_HEAD && !views_ok) return 0;
    switch (k) {
      case B_HEAD:       // (activation backward: this kernel only)
        if (mode == 3) return bp_bf16_head_stats_workspace(g, in, out, mode);
        break;
      case B_FLAT:
        if (bp_bf16_flat_ok(g, in, out, nullptr, mode)) return bp_bf16_flat_stats_workspace(g, in, out, mode);
        break;
      case B_WS:         // (mode 1 only; the larger of the two: bp_set_option may switch kernels later)
        if (mode == 1 && bp_bf16_ws_ok(g, in, out, nullptr, mode)) {
          const size_t ws = bp_bf16_ws_stats_workspace(g, in, out);
          const size_t generic = bp_stats_rows_bytes(bf16_stat_rows(g, c, in, out), g.cout_g);
          return ws > generic ? ws : generic;
        }
        break;
      case B_GENERIC:    // (mode 1 only)
        return mode == 1 ? bp_stats_rows_bytes(bf16_stat_rows(g, c, in, out), g.cout_g) : 0;
    }
  }
  return 0;
}

int bp_bf16_igemm_run(const ConvGeom& g, const bp_view* in, const PW& pw, const void* packed, const float* bias,
                      const bp_view* out, hipStream_t st, const IgemmStatsReq* sr) {
  const BConfig c = b_config(g);
  if (!c.ok) return BP_EUNSUPPORTED;
  const u16* image = reinterpret_cast<const u16*>(packed);
  const BLayout l = bf16_layout(g, c);
  const int mode = sr ? sr->mode : 0;
  const bool views_ok = bp_bf16_igemm_ok(g, in, out);
  for (const BKernel k : B_ORDER) {
    if (k != B_HEAD && !views_ok) return BP_EUNSUPPORTED;
    switch (k) {
      case B_HEAD:      // (it reads its one gathered channel with scalar loads: any channel stride)
        if (!pw.scale && bp_bf16_head_ok(g, in, out, bias, mode)) return bp_bf16_head_run(g, in, image + l.head, out, st, sr);
        break;
      case B_FLAT:
        if (bp_bf16_flat_ok(g, in, out, bias, mode)) return bp_bf16_flat_run(g, in, pw, image + l.flat, out, st, sr);
        break;
      case B_WS:
        if (bp_bf16_ws_ok(g, in, out, bias, mode)) {
          // (the query answers for the generic kernel too, which bp_set_option may bring back: the caller is held to it)
          if (sr && sr->ws_bytes < bp_bf16_stats_workspace(g, in, out, mode)) return BP_EWORKSPACE;
          return bp_bf16_ws_run(g, in, pw, image + l.ws, out, st, sr);
        }
        break;
      case B_GENERIC: break;      // (below)
    }
  }
  BArgs a{};
  a.in = in->ptr; a.in_h = in->h; a.in_w = in->w; a.in_cs = in->cstride; a.in_co = in->coff; a.cin = g.cin_g;
  a.out = out->ptr; a.out_h = out->h; a.out_w = out->w; a.out_cs = out->cstride; a.out_co = out->coff;
  a.cout = g.cout_g; a.wp = image + l.generic; a.bias = bias; a.pw = pw;
  a.tapsy = g.taps; a.ISy = g.IS; a.ISx = g.IS; a.OS = g.OS; a.nphase = g.nphase;
  a.transposed = g.gather_transposed; a.stride = g.stride; a.pad = g.pad;
  a.nrun = c.nrun;
  for (int s = 0; s < c.nrun; ++s) a.run_off[s] = c.run_xm[s] * c.IWq + c.run_xq[s];
  a.TPR = c.TPR; a.BH = c.BH; a.IH = c.IH; a.IWq = c.IWq; a.npixp = c.npixp;
  a.nchunk = c.nchunk; a.cout_padP = c.cout_padP;
  const int qh = bp_ceil_div(out->h, g.OS), qw = bp_ceil_div(out->w, g.OS);
  a.tiles_x = bp_ceil_div(qw, 16 * c.TPR);
  a.tiles_y = bp_ceil_div(qh, c.BH);
  const int64_t gz = (int64_t)in->n * g.nphase * g.nphase;
  if (gz > 65535 || c.cout_padP / c.COB > 65535) return BP_EUNSUPPORTED;
  dim3 grid((unsigned)(a.tiles_x * a.tiles_y), (unsigned)gz, (unsigned)(c.cout_padP / c.COB));
  const bool ib = in->dtype == BP_BF16, ob = out->dtype == BP_BF16;
  const int64_t rows = (int64_t)grid.x * grid.y;
  if (sr) {
    const size_t need = bp_stats_rows_bytes(rows, g.cout_g);
    if (bias || sr->mode != 1 || !need) return BP_EUNSUPPORTED;
    if (!sr->ws || sr->ws_bytes < need || !sr->sums) return BP_EWORKSPACE;
    a.stat = reinterpret_cast<double*>(sr->ws); a.stat_c = g.cout_g;
  }
  int rc = BP_EUNSUPPORTED;
  switch (c.CC) {
    case 32: rc = bp_bf16_launch_cc32(c, a, ib, ob, grid, st); break;
    case 16: rc = bp_bf16_launch_cc16(c, a, ib, ob, grid, st); break;
    case 8: rc = bp_bf16_launch_cc8(c, a, ib, ob, grid, st); break;
    case 4: rc = bp_bf16_launch_cc4(c, a, ib, ob, grid, st); break;
  }
  if (rc != BP_OK || !sr) return rc;
  return bp_stats_rows_finish(a.stat, rows, g.cout_g, sr, st);
}

