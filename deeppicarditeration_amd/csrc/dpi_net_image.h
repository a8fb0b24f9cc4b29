// The device image of a network, built on the host: the argument checks, the weight blob and the
// descriptor (dpi_net_s: NetDev / NetGen / NetGenHead / NetPisDev and the spec / gen / head / term
// flags) of every net kind.  Pure host arithmetic, no HIP runtime call: dpi_net.hip uploads the blob
// and binds the descriptor to the device address, tests/net_image_host.hip binds it to the blob
// itself and reads the image through the descriptor the kernels get.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dpi_host.h"

#include "dpi_dispatch.h"
#include "dpi_pisnet.h"

namespace {

// The same fragment order for the split-storage GEMM (k_gemm_x3, dpi_gemm.h): x' = 2^s x with
// max |x'| in [0.5, 1), hi = fp16(x'), lo = fp16(x' - hi) (unscaled).  *wscale = 2^-s.

// Fragment-major copy of a packed split matrix (R rows of C words, R % 16 == 0, C % 32 == 0) for
// k_pis_net: block (T, c) of 512 words = lane l's hi granule (row 16 T + l % 16, words
// 32 c + 8 (l / 16) .. + 3) at 4 l, then its lo granule (the next 4 words) at 256 + 4 l.
static size_t pack_frag_major(std::vector<float>& blob, size_t src, int R, int C) {
  blob.resize((blob.size() + 31) & ~size_t(31), 0.f);
  const size_t off = blob.size();
  blob.resize(off + (size_t)R * C, 0.f);
  const int nc = C / 32;
  for (int T = 0; T < R / 16; ++T)
    for (int c = 0; c < nc; ++c)
      for (int h = 0; h < 2; ++h)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 4; ++j)
            blob[off + (((size_t)T * nc + c) * 2 + h) * 256 + 4 * l + j] =
                blob[src + (size_t)(16 * T + (l & 15)) * C + 32 * c + 8 * (l >> 4) + 4 * h + j];
  return off;
}

template <class F>
static size_t pack_split_x3(std::vector<float>& blob, int R, int C, F at, float* wscale) {
  float mx = 0.f;
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) mx = std::max(mx, std::fabs(at(r, c)));
  int e = 0;
  if (mx > 0.f) (void)std::frexp(mx, &e);  // mx = f 2^e, f in [0.5, 1)
  const float sc = std::ldexp(1.0f, -e);
  *wscale = std::ldexp(1.0f, e);
  const size_t off = blob.size();
  blob.resize(off + (size_t)R * C, 0.f);
  _Float16* dst = reinterpret_cast<_Float16*>(blob.data() + off);
  for (int r = 0; r < R; ++r)
    for (int u = 0; u < C / 32; ++u)
      for (int q = 0; q < 4; ++q) {
        _Float16* g = dst + ((size_t)r * C + 32 * u + 8 * q) * 2;  // 16 halves = 8 words
        for (int j = 0; j < 8; ++j) {
          const float x = at(r, 32 * u + 4 * q + (j & 3) + 16 * (j >> 2)) * sc;
          const _Float16 h = (_Float16)x;
          g[j] = h;
          g[8 + j] = (_Float16)(x - (float)h);
        }
      }
  return off;
}

// Append an R x C (C % 32 == 0) matrix in the fp16-split fragment order of mlp_tile_split:
// row r, chunk u, lane group q: 8 hi halves then 8 lo halves of columns 32u + 4q + (j & 3) + 16 (j >> 2).
// Returns the offset (in 4-byte words) into `blob`.
template <class F>
static size_t pack_split(std::vector<float>& blob, int R, int C, F at) {
  const size_t off = blob.size();
  blob.resize(off + (size_t)R * C, 0.f);
  _Float16* dst = reinterpret_cast<_Float16*>(blob.data() + off);
  for (int r = 0; r < R; ++r)
    for (int u = 0; u < C / 32; ++u)
      for (int q = 0; q < 4; ++q) {
        _Float16* g = dst + ((size_t)r * C + 32 * u + 8 * q) * 2;  // 16 halves = 8 words
        for (int j = 0; j < 8; ++j) {
          const float x = at(r, 32 * u + 4 * q + (j & 3) + 16 * (j >> 2));
          const _Float16 h = (_Float16)x;
          g[j] = h;
          g[8 + j] = (_Float16)((x - (float)h) * 2048.0f);
        }
      }
  return off;
}

// ---------------------------------------------------------------- operand exponents (split storage)
// A value stored split with an unscaled residual, hi = fp16(v), lo = fp16(v - hi) (the x3 convention
// of k_gemm_x3 / k_pis_net / k_pis_time and of the GBM tangent sweep), keeps fp32's relative precision
// only while lo is an fp16 normal (|v| >~ 2^-2); below that its error is absolute, ~2^-25.  A network
// with small weights makes every activation (or cotangent, or tangent) of a layer small, and the
// products that read them then lose precision that exact fp32 keeps (tools/probe_small.py "homog").
// So every such operand is stored as 2^e v, e per operand and network, chosen on the host from a
// calibration pass of the network itself (double precision, fixed synthetic inputs) so that the
// operand's rms is ~4: per element fp32-class down to ~rms/16, 2^14 of headroom above the rms before
// fp16 overflows (the range guard's case).  The consuming product folds 2^-e into its weight scale,
// so the arithmetic is a power of two per operand — exact.
static int x3_exponent(double sumsq, double count) {
  if (!(count > 0) || !(sumsq > 0) || !std::isfinite(sumsq)) return 0;
  const int e = 2 - (int)std::lround(0.5 * std::log2(sumsq / count));
  return std::min(std::max(e, -40), 40);
}
// fixed-seed N(0, 1) calibration inputs (splitmix64 + Box-Muller; host only, not a label draw)
struct CalNormal {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  double u01() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return ((double)((z ^ (z >> 31)) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  }
  double operator()() { return std::sqrt(-2.0 * std::log(u01())) * std::cos(6.283185307179586 * u01()); }
};
constexpr int CAL_ROWS = 16;
static double cal_act(int act, double z) { return act == DPI_ACT_TANH ? std::tanh(z) : (z > 0 ? z : std::expm1(z)); }
static double cal_dact(int act, double a) { return act == DPI_ACT_TANH ? 1.0 - a * a : (a > 0 ? 1.0 : a + 1.0); }
// y = W x + b (W row-major (o, in)); b may be null
static void cal_affine(const float* W, const float* b, int o, int in, const double* x, double* y) {
  for (int r = 0; r < o; ++r) {
    double a = b ? (double)b[r] : 0.0;
    const float* w = W + (size_t)r * in;
    for (int k = 0; k < in; ++k) a += (double)w[k] * x[k];
    y[r] = a;
  }
}
// y = W^T x (W row-major (o, in), x of length o)
static void cal_affine_t(const float* W, int o, int in, const double* x, double* y) {
  for (int k = 0; k < in; ++k) y[k] = 0.0;
  for (int r = 0; r < o; ++r) {
    const float* w = W + (size_t)r * in;
    for (int k = 0; k < in; ++k) y[k] += (double)w[k] * x[r];
  }
}

// PISGradNet's operand exponents: t_encoder's hidden layer (te) and output (temb), the operand of
// smooth_net block j (sn[j]), nn_module's activations A_l (a[l]) and VJP cotangents D_l (d[l]).
// Calibration rows: lambda evenly over (0, T), X ~ N(0, 4 I) (the OU/HJB state scale, x ~ N(0, (4 + t) I)).
struct PisExps {
  int te, temb, sn[4], a[4], d[4];
};
static PisExps pis_calibrate(int nx, int L, const int* hidden, double T, const float* phase, const float* coeff,
                             const float* te0, const float* te0b, const float* te2, const float* te2b, const float* sn0,
                             const float* sn0b, const float* const* snw, const float* const* snbw, int nsm,
                             const float* const* nnw, const float* const* nnbw, const int* ins) {
  const int C = PIS_CH;
  double s_te = 0, s_temb = 0, s_sn[4] = {0, 0, 0, 0}, s_a[4] = {0, 0, 0, 0}, s_d[4] = {0, 0, 0, 0};
  int hmax = C;
  for (int l = 0; l < L; ++l) hmax = std::max(hmax, hidden[l]);
  std::vector<double> e(2 * C), h(C), h2(C), in0(C + nx), A[4], D(hmax), D2(hmax);
  for (int l = 0; l < L; ++l) A[l].assign(hidden[l], 0.0);
  CalNormal nrm;
  auto sq = [](const std::vector<double>& v, int n) {
    double s = 0;
    for (int k = 0; k < n; ++k) s += v[k] * v[k];
    return s;
  };
  for (int r = 0; r < CAL_ROWS; ++r) {
    const double lbd = T * (r + 0.5) / CAL_ROWS;
    for (int j = 0; j < C; ++j) {
      const double a = (double)coeff[j] * lbd + (double)phase[j];
      e[j] = std::sin(a);
      e[C + j] = std::cos(a);
    }
    cal_affine(te0, te0b, C, 2 * C, e.data(), h.data());
    for (int k = 0; k < C; ++k) h[k] = cal_act(DPI_ACT_ELU, h[k]);
    s_te += sq(h, C);
    cal_affine(te2, te2b, C, C, h.data(), in0.data());
    for (int k = 0; k < C; ++k) s_temb += in0[k] * in0[k];
    cal_affine(sn0, sn0b, C, 2 * C, e.data(), h.data());
    for (int j = 0; j < nsm; ++j) {
      for (int k = 0; k < C; ++k) h[k] = cal_act(DPI_ACT_ELU, h[k]);
      s_sn[j] += sq(h, C);
      cal_affine(snw[j], snbw[j], C, C, h.data(), h2.data());
      h.swap(h2);
    }
    for (int d = 0; d < nx; ++d) in0[C + d] = 2.0 * nrm();
    const double* x = in0.data();
    for (int l = 0; l < L; ++l) {
      cal_affine(nnw[l], nnbw[l], hidden[l], ins[l], x, A[l].data());
      for (int k = 0; k < hidden[l]; ++k) A[l][k] = cal_act(DPI_ACT_ELU, A[l][k]);
      s_a[l] += sq(A[l], hidden[l]);
      x = A[l].data();
    }
    // VJP with cotangent X on net_out: D_{L-1} = (nn_L^T X) elu'(A_{L-1}), D_{l-1} = (nn_l^T D_l) elu'(A_{l-1})
    cal_affine_t(nnw[L], nx, ins[L], in0.data() + C, D.data());
    for (int l = L - 1; l >= 0; --l) {
      for (int k = 0; k < hidden[l]; ++k) D[k] *= cal_dact(DPI_ACT_ELU, A[l][k]);
      s_d[l] += sq(D, hidden[l]);
      if (l > 0) {
        cal_affine_t(nnw[l], hidden[l], ins[l], D.data(), D2.data());
        D.swap(D2);
      }
    }
  }
  PisExps x;
  x.te = x3_exponent(s_te, (double)CAL_ROWS * C);
  x.temb = x3_exponent(s_temb, (double)CAL_ROWS * C);
  for (int j = 0; j < 4; ++j) x.sn[j] = j < nsm ? x3_exponent(s_sn[j], (double)CAL_ROWS * C) : 0;
  for (int l = 0; l < 4; ++l) {
    x.a[l] = l < L ? x3_exponent(s_a[l], (double)CAL_ROWS * hidden[l]) : 0;
    x.d[l] = l < L ? x3_exponent(s_d[l], (double)CAL_ROWS * hidden[l]) : 0;
  }
  return x;
}

// The MLP tangent sweep's operand exponents (mlp_hdiag_split): activations a_l (the forward's B
// operands of layers l + 1) and tangent operands act'(a_l) z_l, z_0 = W1x[:, d] over every direction d
// (z_{l+1} = W_{l+1} (act'(a_l) z_l)).  Calibration rows: t evenly over (0, T), x ~ N(0, I).
static void mlp_calibrate(int nx, int H, int L, int act, const float* W0, const float* b0, const float* const* W,
                          const float* const* b, int* ea, int* eb) {
  const int n_in = 1 + nx;
  double sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
  std::vector<double> x(n_in), a[4], z((size_t)H * nx), zn((size_t)H * nx);
  for (int l = 0; l < L; ++l) a[l].assign(H, 0.0);
  CalNormal nrm;
  for (int r = 0; r < CAL_ROWS; ++r) {
    x[0] = (r + 0.5) / CAL_ROWS;
    for (int d = 0; d < nx; ++d) x[1 + d] = nrm();
    cal_affine(W0, b0, H, n_in, x.data(), a[0].data());
    for (int k = 0; k < H; ++k) a[0][k] = cal_act(act, a[0][k]);
    for (int l = 1; l < L; ++l) {
      cal_affine(W[l], b[l], H, H, a[l - 1].data(), a[l].data());
      for (int k = 0; k < H; ++k) a[l][k] = cal_act(act, a[l][k]);
    }
    for (int l = 0; l + 1 < L; ++l)
      for (int k = 0; k < H; ++k) sa[l] += a[l][k] * a[l][k];
    if (r >= 4) continue;  // the tangents (H^2 nx per layer) from the first 4 rows
    // tangents of every direction at once: z[h][d]
    for (int h = 0; h < H; ++h)
      for (int d = 0; d < nx; ++d) z[(size_t)h * nx + d] = W0[(size_t)h * n_in + 1 + d];
    for (int l = 0; l + 1 < L; ++l) {
      for (int h = 0; h < H; ++h) {
        const double f = cal_dact(act, a[l][h]);
        for (int d = 0; d < nx; ++d) {
          z[(size_t)h * nx + d] *= f;
          sb[l] += z[(size_t)h * nx + d] * z[(size_t)h * nx + d];
        }
      }
      std::fill(zn.begin(), zn.end(), 0.0);
      for (int o = 0; o < H; ++o)
        for (int k = 0; k < H; ++k) {
          const double w = W[l + 1][(size_t)o * H + k];
          if (w != 0.0)
            for (int d = 0; d < nx; ++d) zn[(size_t)o * nx + d] += w * z[(size_t)k * nx + d];
        }
      z.swap(zn);
    }
  }
  for (int l = 0; l < 4; ++l) {
    ea[l] = l + 1 < L ? x3_exponent(sa[l], (double)CAL_ROWS * H) : 0;
    eb[l] = l + 1 < L ? x3_exponent(sb[l], 4.0 * H * nx) : 0;
  }
}

// ---------------------------------------------------------------- the blob and the descriptor
// The weight blob: fp32 words; every region starts on a multiple of 4 words (16 B), the split-storage
// regions of a PISGradNet on a multiple of 32 (align).  Each call returns its region's word offset.
struct NetBlob {
  std::vector<float> v;
  size_t take(size_t cnt) {  // cnt zero words
    const size_t off = v.size();
    v.resize(off + ((cnt + 3) & ~size_t(3)), 0.f);
    return off;
  }
  size_t put(const float* src, size_t cnt) {
    const size_t off = take(cnt);
    std::memcpy(v.data() + off, src, cnt * sizeof(float));
    return off;
  }
  size_t putT(const float* src, int rows, int cols, int c0, int nc) {  // (src[:, c0:c0+nc])^T
    const size_t off = take((size_t)nc * rows);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < nc; ++c) v[off + (size_t)c * rows + r] = src[(size_t)r * cols + c0 + c];
    return off;
  }
  void align() { v.resize((v.size() + 31) & ~size_t(31), 0.f); }
};

// A built image: the blob and its descriptor.  Until net_bind, a pointer field of the descriptor
// holds its region's word offset in the blob plus one, as an integer (0: the net has no such region).
struct NetImage {
  std::vector<float> blob;
  dpi_net_s net{};
};
template <class T>
void set_off(const T*& p, size_t off) {
  p = reinterpret_cast<const T*>(uintptr_t(off + 1));
}
template <class T>
size_t get_off(const T* p) {
  return reinterpret_cast<uintptr_t>(p) - 1;
}
template <class T>
void bind_ptr(const T*& p, const float* base) {
  if (p) p = reinterpret_cast<const T*>(base + get_off(p));
}
template <class Net>  // the dense image's fields: NetDev and NetGen name them alike
void bind_dense(Net& n, const float* base) {
  bind_ptr(n.W1x, base), bind_ptr(n.w1t, base), bind_ptr(n.b1, base), bind_ptr(n.c1, base), bind_ptr(n.W1xT, base);
  for (auto& p : n.W) bind_ptr(p, base);
  for (auto& p : n.WT) bind_ptr(p, base);
  for (auto& p : n.b) bind_ptr(p, base);
  bind_ptr(n.wout, base);
}
// Point every region pointer of the descriptor into the blob's copy at `base` (once per descriptor).
void net_bind(dpi_net_s& n, const float* base) {
  bind_dense(n.d, base), bind_dense(n.g, base), bind_dense(n.hd, base);
  bind_ptr(n.hd.G, base), bind_ptr(n.hd.bg, base);
  bind_ptr(n.d.W1xS, base), bind_ptr(n.d.W1xTS, base);
  for (int l = 0; l < 4; ++l) bind_ptr(n.d.WS[l], base), bind_ptr(n.d.WTS[l], base), bind_ptr(n.d.WU[l], base);
  NetPisDev& p = n.pis;
  for (auto q : {&p.phase, &p.coeff, &p.te0, &p.te0b, &p.te2, &p.te2b, &p.sn0, &p.sn0b, &p.snlast, &p.snlastb})
    bind_ptr(*q, base);
  for (auto q : {&p.te0S, &p.te2S, &p.sn0S, &p.gxnoS, &p.gxnoF}) bind_ptr(*q, base);
  for (int j = 0; j < 4; ++j) bind_ptr(p.sn[j], base), bind_ptr(p.snb[j], base), bind_ptr(p.snS[j], base);
  for (int l = 0; l < 5; ++l) {
    bind_ptr(p.nn[l], base), bind_ptr(p.nnb[l], base), bind_ptr(p.nnT[l], base), bind_ptr(p.nnbP[l], base);
    bind_ptr(p.nnS[l], base), bind_ptr(p.nnTS[l], base), bind_ptr(p.nnF[l], base), bind_ptr(p.nnTF[l], base);
  }
}

// ---------------------------------------------------------------- MLP nets
// One Linear as the caller's parameter vector holds it: W row-major (rows, cols), then b (rows).
struct DenseLayer {
  int rows, cols;
  const float *W, *b;
};

// The dense fp32 image of a net's hidden layers ly[0..L) (ly[0]: (rows, 1 + nx)) and its value row
// wout (ly[L - 1].rows words; null: zeros), zero-padded to the row stride S:
//   W1x (S, nxp) | w1t (S) | b1 (S) | c1 (S) | W1xT (nxpT, S) | [W[l] (S, S) | WT[l] (S, S) | b[l] (S)], l = 1..L-1 | wout (S)
// c1[h] = sum_d W1x[h][d], summed in fp64 in the order of d.  A padded unit has zero weights and bias
// in and zero weights out, so its activation (ELU(0) = tanh(0) = 0) and every gradient through it add
// exact zeros: the labels are those of the unpadded network.
template <class Net>
void pack_dense(NetBlob& B, Net& n, const DenseLayer* ly, int L, const float* wout, int nx, int S, int nxp, int nxpT) {
  std::vector<float>& v = B.v;
  const size_t W1x = B.take((size_t)S * nxp), w1t = B.take(S), b1 = B.take(S), c1 = B.take(S),
               W1xT = B.take((size_t)nxpT * S);
  for (int h = 0; h < ly[0].rows; ++h) {
    const float* row = ly[0].W + (size_t)h * (1 + nx);
    double cs = 0;
    for (int d = 0; d < nx; ++d) {
      const float w = row[1 + d];
      v[W1x + (size_t)h * nxp + d] = w;
      v[W1xT + (size_t)d * S + h] = w;
      cs += w;
    }
    v[w1t + h] = row[0];
    v[b1 + h] = ly[0].b[h];
    v[c1 + h] = (float)cs;
  }
  set_off(n.W1x, W1x), set_off(n.w1t, w1t), set_off(n.b1, b1), set_off(n.c1, c1), set_off(n.W1xT, W1xT);
  for (int l = 1; l < L; ++l) {
    const size_t W = B.take((size_t)S * S), WT = B.take((size_t)S * S), b = B.take(S);
    for (int r = 0; r < ly[l].rows; ++r) {
      for (int c = 0; c < ly[l].cols; ++c) {
        v[W + (size_t)r * S + c] = ly[l].W[(size_t)r * ly[l].cols + c];
        v[WT + (size_t)c * S + r] = ly[l].W[(size_t)r * ly[l].cols + c];
      }
      v[b + r] = ly[l].b[r];
    }
    set_off(n.W[l], W), set_off(n.WT[l], WT), set_off(n.b[l], b);
  }
  const size_t wo = B.take(S);
  if (wout) std::memcpy(v.data() + wo, wout, ly[L - 1].rows * sizeof(float));
  set_off(n.wout, wo);
}

// The fp16-split copies of a specialised image (H % 32 == 0) for the split MFMA path, read from the
// dense image already in the blob, and mlp_hdiag_split's operand scales.
void pack_mlp_split(NetBlob& B, NetDev& d, int nx) {
  const int H = d.H, L = d.L, nxp = d.nxp, nxp32 = d.nxp32, n_in = 1 + nx;
  std::vector<float>& v = B.v;
  size_t oW[4] = {get_off(d.W1x)};
  for (int l = 1; l < L; ++l) oW[l] = get_off(d.W[l]);
  auto Wx = [&](int h, int dd) { return dd < nx ? v[oW[0] + (size_t)h * nxp + dd] : 0.f; };
  set_off(d.W1xS, pack_split(v, H, nxp32, Wx));
  set_off(d.W1xTS, pack_split(v, nxp32, H, [&](int dd, int h) { return Wx(h, dd); }));
  for (int l = 1; l < L; ++l) {
    auto Wl = [&](int r, int c) { return v[oW[l] + (size_t)r * H + c]; };
    set_off(d.WS[l], pack_split(v, H, H, Wl));
    set_off(d.WTS[l], pack_split(v, H, H, [&](int r, int c) { return Wl(c, r); }));
    set_off(d.WU[l], pack_split_x3(v, H, H, Wl, &d.wus[l]));
  }
  // the calibration pass reads the padded network: layer 1 as (H, n_in) rows, the rest in place
  std::vector<float> W0((size_t)H * n_in);
  for (int h = 0; h < H; ++h) {
    W0[(size_t)h * n_in] = v[get_off(d.w1t) + h];
    for (int dd = 0; dd < nx; ++dd) W0[(size_t)h * n_in + 1 + dd] = Wx(h, dd);
  }
  const float *Wl[4] = {nullptr, nullptr, nullptr, nullptr}, *bl[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int l = 1; l < L; ++l) Wl[l] = v.data() + oW[l], bl[l] = v.data() + get_off(d.b[l]);
  int ea[4], eb[4];
  mlp_calibrate(nx, H, L, d.act, W0.data(), v.data() + get_off(d.b1), Wl, bl, ea, eb);
  // mlp_hdiag_split: forward operand of layer l + 1 = 2^ea[l] a_l, tangent operand = 2^eb[l] act'(a_l) z_l
  for (int l = 0; l < L; ++l) {
    d.hsa[l] = std::ldexp(1.0f, ea[l]);
    if (l >= 1) d.hsc[l] = std::ldexp(d.wus[l], -ea[l - 1]);
    d.hzs[l] = l == 0 ? 1.0f : std::ldexp(d.wus[l], -eb[l - 1]);
    d.hbs[l] = l == 0 ? std::ldexp(1.0f, eb[0]) : std::ldexp(d.wus[l], eb[l] - eb[l - 1]);
  }
}

// What dpi_net_create_mlp{,_head,_terminal} ask for beyond the layers: the last Linear's form
// (DPI_HEAD_*) and whether the net is read as the terminal-enforcing ansatz of horizon T.
struct MlpSpec {
  int head = DPI_HEAD_VALUE;
  bool term = false;
  double T = 0.0;
};

// The argument checks of every MLP net, value and head alike.
int mlp_check(int n_in, int n_hidden, const int* widths, int act, int head, const float* params, size_t n_params,
              const void* out) {
  if (n_in - 1 > NXW_MAX)
    return fail(DPI_ERR_UNSUPPORTED, "mlp: nx = n_in - 1 exceeds the compiled maximum state dimension 256 (NXW_MAX)");
  if (!out || !widths || !params || n_in < 2 || n_hidden < 1) return fail(DPI_ERR_ARG, "mlp: bad arguments");
  if (n_hidden > GEN_LMAX) return fail(DPI_ERR_UNSUPPORTED, "mlp: at most 8 hidden layers (GEN_LMAX)");
  if (act != DPI_ACT_ELU && act != DPI_ACT_TANH)
    return fail(DPI_ERR_UNSUPPORTED, "mlp: activations must be DPI_ACT_ELU or DPI_ACT_TANH");
  if (head != DPI_HEAD_VALUE && head != DPI_HEAD_VALUE_GRADIENT && head != DPI_HEAD_GRADIENT)
    return fail(DPI_ERR_ARG, "mlp_head: head must be DPI_HEAD_VALUE, DPI_HEAD_VALUE_GRADIENT or DPI_HEAD_GRADIENT");
  size_t expect = 0;
  for (int l = 0; l < n_hidden; ++l) {
    if (widths[l] < 1 || widths[l] > GEN_HMAX)
      return fail(DPI_ERR_UNSUPPORTED, "mlp: hidden widths must be in [1, 256] (GEN_HMAX)");
    expect += (size_t)widths[l] * ((l ? widths[l - 1] : n_in) + 1);
  }
  const int n_out = head == DPI_HEAD_VALUE ? 1 : head == DPI_HEAD_VALUE_GRADIENT ? n_in : n_in - 1;
  expect += (size_t)n_out * (widths[n_hidden - 1] + 1);
  if (n_params != expect)
    return fail(DPI_ERR_ARG, head == DPI_HEAD_VALUE ? "mlp: parameter count mismatch"
                             : head == DPI_HEAD_VALUE_GRADIENT
                                 ? "mlp_head: parameter count mismatch (a ValueGradient head has 1 + nx output rows)"
                                 : "mlp_head: parameter count mismatch (an OnlyGradient head has nx output rows)");
  return 0;
}

// The image of an MLP net that passed mlp_check.  Any hidden widths up to 256, up to 8 layers.  A value
// net of up to 4 layers of widths <= 128 gets the specialised image (NetDev): the layers zero-padded to
// the smallest compiled width H in {16, 32, 64, 128} that holds the widest one.  A net without a
// specialised first-order Cha / OU instance of its (H, L) also (or only) gets the general family's
// image (NetGen), padded the same way to 128 or 256; a terminal-enforcing value net has no specialised
// instance, whatever its shape.  A gradient-head net gets the general image only, as NetGenHead.
void build_mlp(NetImage& img, int n_in, int n_hidden, const int* widths, int act, const MlpSpec& s,
               const float* params) {
  const int nx = n_in - 1, L = n_hidden;
  DenseLayer ly[GEN_LMAX];
  const float* q = params;
  int wmax = 0;
  for (int l = 0; l < L; ++l) {
    const int win = l ? widths[l - 1] : n_in;
    ly[l] = {widths[l], win, q, q + (size_t)widths[l] * win};
    q += (size_t)widths[l] * (win + 1);  // then q: the last Linear
    wmax = std::max(wmax, widths[l]);
  }
  const int wl = widths[L - 1];
  const int H = wmax <= 16 ? 16 : wmax <= 32 ? 32 : wmax <= 64 ? 64 : wmax <= 128 ? 128 : 256;
  const int HC = H <= 128 ? 128 : 256, nxg = (nx + 15) & ~15, nxg32 = (nx + 31) & ~31;
  const bool headed = s.head != DPI_HEAD_VALUE;
  const bool spec = !headed && !s.term && L <= 4 && wmax <= HMAX;
  const bool gen = !spec || !spec_shape(DPI_EQ_CHA, H, L);  // Cha and OU share a list
  // nx padded to 16 (the fp32 weight images) and to 32 (the split ones).  The split layer-1 rows are
  // LDS chunks of at most 128 words whose 16-B granules are XOR-swizzled by row (split_swz): a closed
  // permutation only for 8, 16 or 32 granules per row, so a chunk of 96 words (nx in 65..96, or
  // 193..224 in the wide instances) is padded to 128 with zero columns — and nxp with it, so the path
  // kernels zero those rows of their noise tile (and the fp32 images carry the same zero columns)
  int nxp = (nx + 15) & ~15, nxp32 = (nx + 31) & ~31;
  if ((nxp32 & 127) == 96) nxp = nxp32 = nxp32 + 32;
  NetBlob B;
  dpi_net_s& n = img.net;
  n.n_in = n_in;
  n.spec = spec, n.gen = gen, n.head = s.head;
  n.term = s.term, n.term_T = s.term ? (float)s.T : 0.f;
  n.d.kind = 1, n.d.L = L, n.d.act = act;
  n.d.H = headed ? HC : H, n.d.nxp = headed ? nxg : nxp;
  NetGen& g = headed ? n.hd : n.g;
  if (gen) g.H = HC, g.L = L, g.nxp = nxg, g.act = act, g.ht = ((wmax + 31) & ~31) / 16;
  if (headed) {
    // the last Linear: [value row |] nx gradient rows, then their biases; c1 holds cg[h] = sum_d G[d][h],
    // and bgsum = sum_d bg[d], both summed in fp64
    NetGenHead& hd = n.hd;
    const bool value = s.head == DPI_HEAD_VALUE_GRADIENT;
    const float* const Wg = q + (value ? wl : 0);
    const float* const bo = q + (size_t)(value ? 1 + nx : nx) * wl;
    pack_dense(B, hd, ly, L, value ? q : nullptr, nx, HC, nxg, nxg32);
    const size_t cg = get_off(hd.c1), G = B.take((size_t)nxg32 * HC), bg = B.take(nxg32);
    std::fill_n(B.v.begin() + cg, HC, 0.f);
    for (int h = 0; h < wl; ++h) {
      double cs = 0;
      for (int d = 0; d < nx; ++d) {
        const float w = Wg[(size_t)d * wl + h];
        B.v[G + (size_t)d * HC + h] = w;
        cs += w;
      }
      B.v[cg + h] = (float)cs;
    }
    double bs = 0;
    for (int d = 0; d < nx; ++d) {
      B.v[bg + d] = bo[(value ? 1 : 0) + d];
      bs += bo[(value ? 1 : 0) + d];
    }
    set_off(hd.G, G), set_off(hd.bg, bg);
    hd.value = value ? 1 : 0, hd.bout = value ? bo[0] : 0.f, hd.bgsum = (float)bs;
    n.g = hd;  // the NetGen part: what the workspace layout and the routing read
  } else if (gen) {
    pack_dense(B, g, ly, L, q, nx, HC, nxg, nxg32);
    g.bout = q[wl];
  }
  if (spec) {
    pack_dense(B, n.d, ly, L, q, nx, H, nxp, nxp);
    n.d.bout = q[wl];
    n.d.nxp32 = nxp32;
    if (H % 32 == 0) pack_mlp_split(B, n.d, nx);
  }
  img.blob = std::move(B.v);
}

// ---------------------------------------------------------------- PISGradNet
int pisgrad_check(int nx, int n_hidden, const int* hidden, const float* params, size_t n_params, const void* out) {
  if (nx > NXP_MAX)
    return fail(DPI_ERR_UNSUPPORTED, "pisgrad: nx exceeds the compiled maximum state dimension 128 (NXP_MAX)");
  if (!out || !hidden || !params || nx < 1 || n_hidden < 1 || n_hidden > 4)
    return fail(DPI_ERR_ARG, "pisgrad: bad arguments (1 <= n_hidden <= 4, nx <= 128)");
  for (int l = 0; l < n_hidden; ++l)
    if (hidden[l] < 4 || hidden[l] > 1024 || (hidden[l] % 4)) return fail(DPI_ERR_ARG, "pisgrad: hidden widths % 4");
  const int C = PIS_CH;
  // expected parameter count in state-dict order (solution.py:160-205)
  size_t expect = 2 * C + (size_t)C * 2 * C + C + (size_t)C * C + C;                       // phase, coeff, t_encoder
  expect += (size_t)C * 2 * C + C + (size_t)n_hidden * (C * C + C) + (size_t)nx * C + nx;  // smooth_net
  int in = C + nx;
  for (int l = 0; l < n_hidden; ++l) {
    expect += (size_t)hidden[l] * in + hidden[l];
    in = hidden[l];
  }
  expect += (size_t)nx * in + nx;
  if (n_params != expect) return fail(DPI_ERR_ARG, "pisgrad: parameter count mismatch");
  return 0;
}

// The image of a PISGradNet that passed pisgrad_check.
void build_pisgrad(NetImage& img, int nx, int n_hidden, const int* hidden, double T, const float* params) {
  const int C = PIS_CH, nsm = n_hidden, L = n_hidden, IN = C + nx;
  const float* q = params;
  auto take_src = [&](size_t cnt) {
    const float* r = q;
    q += cnt;
    return r;
  };
  const float* phase = take_src(C);
  const float* coeff = take_src(C);
  const float* te0 = take_src((size_t)C * 2 * C);
  const float* te0b = take_src(C);
  const float* te2 = take_src((size_t)C * C);
  const float* te2b = take_src(C);
  const float* sn0 = take_src((size_t)C * 2 * C);
  const float* sn0b = take_src(C);
  const float *snw[4], *snbw[4];
  for (int j = 0; j < nsm; ++j) {
    snw[j] = take_src((size_t)C * C);
    snbw[j] = take_src(C);
  }
  const float* snl = take_src((size_t)nx * C);
  const float* snlb = take_src(nx);
  const float *nnw[5], *nnbw[5];
  int ins[5];
  int in = IN;
  for (int l = 0; l <= L; ++l) {
    const int o = l < L ? hidden[l] : nx;
    nnw[l] = take_src((size_t)o * in);
    nnbw[l] = take_src(o);
    ins[l] = in;
    in = o;
  }
  // smooth0 = smooth_net(emb(0))[0] in double on the host
  double smooth0;
  {
    std::vector<double> e(2 * C), h(C), h2(C);
    for (int j = 0; j < C; ++j) {
      e[j] = std::sin((double)phase[j]);
      e[C + j] = std::cos((double)phase[j]);
    }
    auto elu_d = [](double z) { return z > 0 ? z : std::expm1(z); };
    for (int o = 0; o < C; ++o) {
      double a = sn0b[o];
      for (int k = 0; k < 2 * C; ++k) a += (double)sn0[(size_t)o * 2 * C + k] * e[k];
      h[o] = a;
    }
    for (int j = 0; j < nsm; ++j) {
      for (int o = 0; o < C; ++o) {
        double a = snbw[j][o];
        for (int k = 0; k < C; ++k) a += (double)snw[j][(size_t)o * C + k] * elu_d(h[k]);
        h2[o] = a;
      }
      h.swap(h2);
    }
    double a = snlb[0];
    for (int k = 0; k < C; ++k) a += (double)snl[k] * elu_d(h[k]);
    smooth0 = a;
  }
  const PisExps ex =
      pis_calibrate(nx, L, hidden, T, phase, coeff, te0, te0b, te2, te2b, sn0, sn0b, snw, snbw, nsm, nnw, nnbw, ins);
  NetBlob B;
  std::vector<float>& blob = B.v;
  NetPisDev& pd = img.net.pis;
  pd.nx = nx;
  pd.L = L;
  pd.nsm = nsm;
  for (int l = 0; l < L; ++l) pd.h[l] = hidden[l];
  pd.T = (float)T;
  pd.smooth0 = (float)smooth0;
  set_off(pd.phase, B.put(phase, C)), set_off(pd.coeff, B.put(coeff, C));
  set_off(pd.te0, B.put(te0, (size_t)C * 2 * C)), set_off(pd.te0b, B.put(te0b, C));
  set_off(pd.te2, B.put(te2, (size_t)C * C)), set_off(pd.te2b, B.put(te2b, C));
  set_off(pd.sn0, B.put(sn0, (size_t)C * 2 * C)), set_off(pd.sn0b, B.put(sn0b, C));
  set_off(pd.snlast, B.put(snl, C)), set_off(pd.snlastb, B.put(snlb, 1));
  for (int j = 0; j < nsm; ++j) {
    set_off(pd.sn[j], B.put(snw[j], (size_t)C * C));
    set_off(pd.snb[j], B.put(snbw[j], C));
  }
  for (int l = 0; l <= L; ++l) {
    const int o = l < L ? hidden[l] : nx;
    set_off(pd.nn[l], B.put(nnw[l], (size_t)o * ins[l]));
    set_off(pd.nnb[l], B.put(nnbw[l], o));
    set_off(pd.nnT[l], l == 0 ? B.putT(nnw[0], hidden[0], ins[0], C, nx) : B.putT(nnw[l], o, ins[l], 0, ins[l]));
  }
  // split-storage copies (k_gemm_x3): output dims padded to 64 (hp_l, NOP), input dims to 32
  // (INP = IN's width, NXK = the x part of IN), zero fill, 128-B aligned rows
  auto r64 = [](int x) { return (x + 63) & ~63; };
  const int INP = (C + nx + 31) & ~31, NXK = (nx + 31) & ~31, NOP = r64(nx);
  int hp[4];
  for (int l = 0; l < L; ++l) hp[l] = r64(hidden[l]);
  size_t s_nn[5] = {0}, s_nnT[5] = {0}, s_gxno = 0;
  auto packm = [&](const float* src, int rows, int cols, int Np, int Kp, bool trans, float* ws) {
    B.align();
    return pack_split_x3(blob, Np, Kp, [&](int r, int c) {
      if (trans) return (c < rows && r < cols) ? src[(size_t)c * cols + r] : 0.f;  // (src^T)[r][c]
      return (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
    }, ws);
  };
  // every product's weight scale carries its stored input's 2^-e (x3_exponent); the VJP's also
  // its output's 2^e (EPI_DELU stores (acc ws) elu'(A))
  set_off(pd.te0S, packm(te0, C, 2 * C, C, 2 * C, false, &pd.te0W));
  set_off(pd.te2S, packm(te2, C, C, C, C, false, &pd.te2W));
  pd.te2W = std::ldexp(pd.te2W, -ex.te);
  set_off(pd.sn0S, packm(sn0, C, 2 * C, C, 2 * C, false, &pd.sn0W));
  for (int j = 0; j < nsm; ++j) {
    set_off(pd.snS[j], packm(snw[j], C, C, C, C, false, &pd.snW[j]));
    pd.snW[j] = std::ldexp(pd.snW[j], -ex.sn[j]);
  }
  // forward: nn[0] (h0 x (64 + nx)), nn[l] (h_l x h_{l-1}), nn[L] (nx x h_{L-1}); nn[0]'s t_emb
  // columns carry t_emb's 2^-e (IN holds [2^e t_emb | X], two operands in one K)
  {
    B.align();
    const float* w0 = nnw[0];
    const int in0 = ins[0], h0 = hidden[0];
    s_nn[0] = pack_split_x3(blob, hp[0], INP, [&](int r, int c) {
      if (r >= h0 || c >= in0) return 0.f;
      return c < C ? std::ldexp(w0[(size_t)r * in0 + c], -ex.temb) : w0[(size_t)r * in0 + c];
    }, &pd.nnW[0]);
  }
  for (int l = 1; l < L; ++l) {
    s_nn[l] = packm(nnw[l], hidden[l], ins[l], hp[l], hp[l - 1], false, &pd.nnW[l]);
    pd.nnW[l] = std::ldexp(pd.nnW[l], -ex.a[l - 1]);
  }
  s_nn[L] = packm(nnw[L], nx, ins[L], NOP, hp[L - 1], false, &pd.nnW[L]);
  pd.nnW[L] = std::ldexp(pd.nnW[L], -ex.a[L - 1]);
  // VJP: nnT[L] = nn[L]^T (h_{L-1} x nx), nnT[l] = nn[l]^T, nnT[0] = nn[0][:, 64:]^T (nx x h0)
  s_nnT[L] = packm(nnw[L], nx, ins[L], hp[L - 1], NXK, true, &pd.nnTW[L]);
  pd.nnTW[L] = std::ldexp(pd.nnTW[L], ex.d[L - 1]);
  for (int l = 1; l < L; ++l) {
    s_nnT[l] = packm(nnw[l], hidden[l], ins[l], hp[l - 1], hp[l], true, &pd.nnTW[l]);
    pd.nnTW[l] = std::ldexp(pd.nnTW[l], ex.d[l - 1] - ex.d[l]);
  }
  {
    B.align();
    const float* w0 = nnw[0];
    const int in0 = ins[0], h0 = hidden[0];
    s_nnT[0] = pack_split_x3(blob, NOP, hp[0], [&](int d, int h) {
      return (d < nx && h < h0) ? w0[(size_t)h * in0 + C + d] : 0.f;
    }, &pd.nnTW[0]);
  }
  {  // [nnT[0] | nn[L]]: row d, columns h < hp0 from nn[0][h][64 + d], then nn[L][d][k]
    B.align();
    const float *w0 = nnw[0], *wl = nnw[L];
    const int in0 = ins[0], h0 = hidden[0], inl = ins[L];
    // K order [A_{L-1} | D_0]: k_pis_net forms the A_{L-1} half while A_{L-1} is still in LDS
    // (the two halves' columns carry 2^-e of A_{L-1} resp. D_0)
    s_gxno = pack_split_x3(blob, NOP, hp[L - 1] + hp[0], [&](int d, int k) {
      if (d >= nx) return 0.f;
      if (k < hp[L - 1]) return k < inl ? std::ldexp(wl[(size_t)d * inl + k], -ex.a[L - 1]) : 0.f;
      k -= hp[L - 1];
      return k < h0 ? std::ldexp(w0[(size_t)k * in0 + C + d], -ex.d[0]) : 0.f;
    }, &pd.gxnoW);
  }
  set_off(pd.gxnoS, s_gxno);
  for (int l = 0; l <= L; ++l) {
    set_off(pd.nnS[l], s_nn[l]), set_off(pd.nnTS[l], s_nnT[l]);
    set_off(pd.nnF[l], pack_frag_major(blob, s_nn[l], l < L ? hp[l] : NOP, l == 0 ? INP : hp[l - 1]));
    set_off(pd.nnTF[l],
            pack_frag_major(blob, s_nnT[l], l == 0 ? NOP : hp[l - 1], l == 0 ? hp[0] : l == L ? NXK : hp[l]));
  }
  set_off(pd.gxnoF, pack_frag_major(blob, s_gxno, NOP, hp[L - 1] + hp[0]));
  for (int l = 0; l <= L; ++l) {
    const int o = l < L ? hidden[l] : nx, op = l < L ? hp[l] : NOP;
    B.align();
    const size_t off = B.take(op);
    std::memcpy(blob.data() + off, nnbw[l], o * sizeof(float));
    set_off(pd.nnbP[l], off);
  }
  pd.xs_te = std::ldexp(1.0f, ex.te);
  pd.xs_temb = std::ldexp(1.0f, ex.temb);
  for (int j = 0; j < 4; ++j) pd.xs_sn[j] = std::ldexp(1.0f, ex.sn[j]);
  for (int l = 0; l < 4; ++l) {
    pd.nnO[l] = std::ldexp(1.0f, ex.a[l]);
    pd.nnA[l] = std::ldexp(1.0f, -ex.a[l]);
  }
  img.net.n_in = 1 + nx;
  img.net.d.kind = 2;
  img.blob = std::move(B.v);
}

}  // namespace
