// C-ABI of include/dpi.h (libdpi_hip.so): problem handles, workspace layout, routing, the
// PISGradNet pipeline host code, the label calls, reduce and finalize kernels.  The network handles
// and their device images: dpi_net.hip, dpi_net_image.h.  Device code: dpi_device.h; the k_paths /
// k_baseline instantiations: one dpi_paths_*.hip unit per row of dpi_route.h's unit table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <type_traits>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <optional>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/dpi.h"
#include "dpi_eq.h"
#include "dpi_rng.h"

#include "dpi_dispatch.h"
#include "dpi_host.h"
#include "dpi_pisnet.h"

namespace dpi {

// Canonical fixed-order sum of `cnt` values (stride `stride`): zero-pad to a power of two
// P2 >= 64 and add as a perfect binary tree in index order.  One wave per column: each lane
// first sums its q = P2/64 consecutive values pairwise in registers, then the 64 lane values
// are combined by an xor butterfly, whose every level adds aligned neighbours — the same tree.
// Splitting the values over G ranks (G and cnt powers of two) and combining the rank results
// with the same function therefore reproduces the single-call sum bit for bit.
__device__ __forceinline__ float tree_sum(const float* __restrict__ p, int cnt, size_t stride) {
  const int lane = threadIdx.x & 63;
  int p2 = 64;
  while (p2 < cnt) p2 <<= 1;
  const int q = p2 >> 6;  // values per lane (<= 16)
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int b = lane * q + j;
    v[j] = (j < q && b < cnt) ? p[(size_t)b * stride] : 0.f;
  }
#pragma unroll
  for (int w = 1; w < 16; w <<= 1)
#pragma unroll
    for (int j = 0; j < 16; j += 2 * w)
      if (j + w < q) v[j] = v[j] + v[j + w];
  float s = v[0];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float other = __shfl_xor(s, o, 64);
    s = (lane & o) ? other + s : s + other;  // always (left + right): identical on both lanes
  }
  return s;
}

// partial [n][nbp][slab_row(F)] -> moments [n][2F] (and, if y != nullptr, the finalized labels).
// torch.clip of the reference (data.py:222): NaN stays NaN (fmaxf alone would return -bound).
__device__ __forceinline__ float clip_label(float v, float bound) {
  return v != v ? v : fminf(fmaxf(v, -bound), bound);
}

// Range guard: a label sum that is not finite while the network's parameters are (status != null
// only then) means the network evaluation left its number format — fp16's 65,504 in the split
// storage of the PISGradNet pipeline, or fp32's range — where the fp64 reference would not.  The
// lane stores DPI_STATUS_NONFINITE into the net's sticky status word (a plain vector store: any
// number of writers store the same value); the host reads it with dpi_net_status.
__device__ __forceinline__ void flag_nonfinite(int* status, float s) {
  if (status && !__builtin_isfinite(s)) *(volatile int*)status = DPI_STATUS_NONFINITE;
}

__global__ __launch_bounds__(256) void k_reduce(const float* __restrict__ partial, int n, int F, int nbp,
                                                float* __restrict__ moments, const float* __restrict__ gx,
                                                float invM, int add_g, float bound, float* __restrict__ y,
                                                int ystride, int* status) {
  // a wave per (point, column): reading the slab's lines from several XCDs costs only duplicate
  // fetches of a 0.9 MB slab, while one workgroup per point serialised the columns (14 vs 4.4 us)
  const int i = blockIdx.x, R = slab_row(F);
  const int c = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= 2 * F) return;
  const float s = tree_sum(partial + (size_t)i * nbp * R + c, nbp, (size_t)R);
  if ((threadIdx.x & 63) == 0) {
    if (c < F) flag_nonfinite(status, s);  // the label sums (a sum of squares may overflow alone)
    moments[(size_t)i * 2 * F + c] = s;
    if (y && c < F) {
      float v = s * invM;
      if (c == 0 && add_g) v += gx[i];
      y[(size_t)i * ystride + c] = clip_label(v, bound);
    }
  }
}

// Offset of Hessian element (d1, d2) in one packed group sum of k_paths' Hessian labels
// (hess_store): upper-triangle 16 x 16 tiles of an NT x NT tiling in row order, tile element
// (r, c) at (r & 3) 64 + (r >> 2) 16 + c; (d1, d2) and (d2, d1) read the same word (symmetric labels).
__device__ __forceinline__ int hess_packed_off(int d1, int d2, int NT) {
  const int a = min(d1, d2), b = max(d1, d2);
  const int I = a >> 4, J = b >> 4, r = a & 15, c = b & 15;
  const int q = I * NT - ((I * (I - 1)) >> 1) + (J - I);
  return q * 256 + (r & 3) * 64 + (r >> 2) * 16 + c;
}

// tree_sum's canonical order in ONE thread: the perfect binary tree, left + right at every level,
// over cnt values zero-padded to P2 = max(64, 2^ceil(log2 cnt)) leaves — bitwise tree_sum's result
// (and every power-of-two sharding of the leaves still reproduces it).  Up to 64 leaves the tree
// runs unrolled in registers; beyond, as a binary counter over the leaves (level l holds the left
// subtree of 2^l leaves until its right sibling completes).
__device__ __forceinline__ float thread_tree(const float* __restrict__ p, int cnt, size_t stride) {
  if (cnt <= 64) {
    float v[64];
#pragma unroll
    for (int b = 0; b < 64; ++b) v[b] = b < cnt ? p[(size_t)b * stride] : 0.f;
#pragma unroll
    for (int w = 1; w < 64; w <<= 1)
#pragma unroll
      for (int b = 0; b < 64; b += 2 * w) v[b] = v[b] + v[b + w];
    return v[0];
  }
  int p2 = 64;
  while (p2 < cnt) p2 <<= 1;
  float st[16], x = 0.f;
#pragma unroll
  for (int l = 0; l < 16; ++l) st[l] = 0.f;
#pragma unroll 4
  for (int b = 0; b < p2; ++b) {
    x = b < cnt ? p[(size_t)b * stride] : 0.f;
    bool carry = true;
#pragma unroll
    for (int l = 0; l < 16; ++l)
      if (carry) {
        if ((b >> l) & 1) {
          x = st[l] + x;
        } else {
          st[l] = x;
          carry = false;
        }
      }
  }
  return x;  // the last leaf's carry reached the root
}

// Hessian block sums [n][nbp][TC] (packed upper-triangle tiles, hess_packed_off) -> hsum [n][nx*nx]
// and y[:, off:off+C] = clip(sum / M).  One thread per packed word: consecutive threads read
// consecutive words of every block (each word read once), sum them in the canonical tree over the
// blocks (thread_tree = tree_sum's order), and store the result at (d1, d2) and (d2, d1) (the
// diagonal tiles' lower halves are skipped: (d1, d2) and (d2, d1) take the upper element, as
// hess_packed_off maps them).  Workgroups are mapped XCD-major: workgroup b runs on XCD b % 8, and an
// XCD's workgroups take whole points (bpp workgroups each), so a point's transposed stores merge
// in one L2 instead of leaving eight XCDs as partial lines.
__global__ __launch_bounds__(256) void k_reduce_hess(const float* __restrict__ hpart, int n, int nx, int NT, int nbp,
                                                     int bpp, float* __restrict__ hsum, float invM, float bound,
                                                     float* __restrict__ y, int ystride, int yoff, int* status) {
  const int TC = NT * (NT + 1) / 2 * 256, C = nx * nx;
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int i = (k / bpp) * 8 + xcd, w = (k % bpp) * 256 + threadIdx.x;
  if (i >= n || w >= TC) return;
  const int q = w >> 8, e = w & 255, r = ((e >> 4) & 3) * 4 + (e >> 6), c = e & 15;
  int I = 0, rq = q;
  while (rq >= NT - I) {
    rq -= NT - I;
    ++I;
  }
  const int J = I + rq, d1 = 16 * I + r, d2 = 16 * J + c;
  if (d1 >= nx || d2 >= nx || (I == J && r > c)) return;
  const float s = thread_tree(hpart + (size_t)i * nbp * TC + w, nbp, (size_t)TC);
  flag_nonfinite(status, s);
  const float v = clip_label(s * invM, bound);
  const size_t o1 = (size_t)d1 * nx + d2, o2 = (size_t)d2 * nx + d1;
  if (hsum) {
    hsum[(size_t)i * C + o1] = s;
    hsum[(size_t)i * C + o2] = s;
  }
  if (y) {
    y[(size_t)i * ystride + yoff + o1] = v;
    y[(size_t)i * ystride + yoff + o2] = v;
  }
}

// Hessian sums (n, C) -> y[:, off:off+C] = clip(sum / M)
__global__ void k_finalize_hess(const float* __restrict__ hsum, int n, int C, float invM, float bound,
                                float* __restrict__ y, int ystride, int yoff) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)n * C) return;
  const size_t i = gid / C, c = gid - i * C;
  y[i * ystride + yoff + c] = clip_label(hsum[gid] * invM, bound);
}

// parts [G][len] -> out [len]
__global__ __launch_bounds__(256) void k_reduce_parts(const float* __restrict__ parts, int G, int len,
                                                      float* __restrict__ out) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= len) return;
  const float s = tree_sum(parts + c, G, (size_t)len);
  if ((threadIdx.x & 63) == 0) out[c] = s;
}

__global__ void k_finalize_y(const float* moments, const float* gx, int n, int F, float invM, int add_g,
                             float bound, float* y, int ystride) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n * F) return;
  const int i = gid / F, c = gid - i * F;
  float v = moments[(size_t)i * 2 * F + c] * invM;
  if (c == 0 && add_g) v += gx[i];
  y[(size_t)i * ystride + c] = clip_label(v, bound);
}

__global__ void k_finalize(const float* moments, const float* gx, int n, int F, float invM, int add_g, float bound,
                           float* y) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n * F) return;
  const int i = gid / F, c = gid - i * F;
  float v = moments[(size_t)i * 2 * F + c] * invM;
  if (c == 0 && add_g) v += gx[i];
  y[gid] = clip_label(v, bound);
}

}  // namespace dpi

template <typename T>
static int upload(dpi_problem_s* p, const std::vector<T>& v, const T** out) {
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, v.size() * sizeof(T) + 16));
  HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  p->dev.push_back(d);
  *out = reinterpret_cast<const T*>(d);
  return 0;
}

extern "C" {

int dpi_abi_version(void) { return DPI_ABI_VERSION; }

// ---- launch timers (dpi_launch_timer_*): start / stop events recorded on the timed path
// launch's own dispatch packet
struct LaunchTimer {
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool recorded = false;
};
static LaunchTimer g_timers[DPI_LAUNCH_TIMERS];
static std::mutex g_timer_mu;
static thread_local int g_timer_armed = -1;

int dpi_launch_timer_arm(int slot) {
  if (slot < 0 || slot >= DPI_LAUNCH_TIMERS) return fail(DPI_ERR_ARG, "launch_timer_arm: slot out of range");
  std::lock_guard<std::mutex> lk(g_timer_mu);
  LaunchTimer& t = g_timers[slot];
  if (!t.t0) {
    HIPCHK(hipEventCreate(&t.t0));
    HIPCHK(hipEventCreate(&t.t1));
  }
  t.recorded = false;
  g_timer_armed = slot;
  return 0;
}

int dpi_launch_timer_ms(int slot, float* ms) {
  if (slot < 0 || slot >= DPI_LAUNCH_TIMERS || !ms) return fail(DPI_ERR_ARG, "launch_timer_ms: bad arguments");
  LaunchTimer& t = g_timers[slot];
  if (!t.recorded) return fail(DPI_ERR_ARG, "launch_timer_ms: no launch recorded on this slot since it was armed");
  HIPCHK(hipEventSynchronize(t.t1));
  HIPCHK(hipEventElapsedTime(ms, t.t0, t.t1));
  return 0;
}

// The armed timer's events for the path launch about to be enqueued (and disarm), or nulls.
static void take_timer(hipEvent_t& t0, hipEvent_t& t1) {
  t0 = t1 = nullptr;
  if (g_timer_armed < 0) return;
  LaunchTimer& t = g_timers[g_timer_armed];
  g_timer_armed = -1;
  t0 = t.t0;
  t1 = t.t1;
  t.recorded = true;
}

int dpi_last_error(char* buf, size_t len) {
  if (buf && len) {
    std::strncpy(buf, g_err.c_str(), len - 1);
    buf[len - 1] = 0;
  }
  return (int)g_err.size();
}

static dpi_problem_s* new_problem(int kind, int nx, double alpha, double T) {
  auto* p = new dpi_problem_s();
  std::memset(&p->e, 0, sizeof(p->e));
  p->e.kind = kind;
  p->e.nx = nx;
  p->e.T = (float)T;
  p->e.alpha = (float)alpha;
  p->e.asq = (float)std::sqrt(alpha);
  p->alpha_init_sqrt = 0.f;
  return p;
}

int dpi_problem_create_cha(int nx, double alpha, double k, double T, dpi_problem* out) {
  if (nx > NXW_MAX) return fail(DPI_ERR_UNSUPPORTED, "cha: nx exceeds the compiled maximum state dimension 256 (NXW_MAX)");
  if (!out || nx < 1 || !(alpha > 0)) return fail(DPI_ERR_ARG, "cha: bad arguments");
  auto* p = new_problem(DPI_EQ_CHA, nx, alpha, T);
  const double kp = k / std::sqrt((double)nx);  // equations.py:285
  const double k_alpha_d = kp * alpha * nx;
  p->e.cha_k = (float)kp;
  p->e.cha_C = (float)((2.0 + kp * k_alpha_d) / (2.0 * k_alpha_d));
  *out = p;
  return 0;
}

int dpi_problem_create_ou(int nx, double alpha, double T, double theta, double mu, double alpha_scale, int n_comp,
                          const double* mean, const double* var_diag, const double* pi, dpi_problem* out) {
  if (nx > NXW_MAX) return fail(DPI_ERR_UNSUPPORTED, "ou: nx exceeds the compiled maximum state dimension 256 (NXW_MAX)");
  if (!out || nx < 1 || n_comp < 1 || n_comp > NSG || !mean || !var_diag || !pi)
    return fail(DPI_ERR_ARG, "ou: bad arguments (1 <= n_comp <= 8, nx <= 256)");
  auto* p = new_problem(DPI_EQ_OU, nx, alpha, T);
  p->e.ou_theta = (float)theta;
  p->e.ou_mu = (float)mu;
  p->e.ou_d = (float)nx;
  p->e.ncomp = n_comp;
  p->alpha_init_sqrt = (float)std::sqrt(alpha_scale * alpha);
  std::vector<float> m(n_comp * nx), iv(n_comp * nx), lc(n_comp);
  const double log2pi = std::log(2.0 * M_PI);
  for (int c = 0; c < n_comp; ++c) {
    double logdet = 0;
    for (int d = 0; d < nx; ++d) {
      m[c * nx + d] = (float)mean[c * nx + d];
      iv[c * nx + d] = (float)(1.0 / var_diag[c * nx + d]);
      logdet += std::log(var_diag[c * nx + d]);
    }
    lc[c] = (float)(std::log(pi[c]) - 0.5 * (nx * log2pi + logdet));
  }
  int rc;
  if ((rc = upload(p, m, &p->e.mean)) || (rc = upload(p, iv, &p->e.ivar)) || (rc = upload(p, lc, &p->e.logc))) {
    delete p;
    return rc;
  }
  *out = p;
  return 0;
}

int dpi_problem_create_gbm(int nx, double alpha, double T, int n_nodes, const double* w, const double* v,
                           dpi_problem* out) {
  if (nx > NXW_MAX) return fail(DPI_ERR_UNSUPPORTED, "gbm: nx exceeds the compiled maximum state dimension 256 (NXW_MAX)");
  if (!out || nx < 1 || n_nodes < 1 || n_nodes > NSG || !w || !v)
    return fail(DPI_ERR_ARG, "gbm: bad arguments (1 <= n_nodes <= 8, nx <= 256)");
  auto* p = new_problem(DPI_EQ_GBM, nx, alpha, T);
  p->e.nodes = n_nodes;
  const int F = 1 + nx;
  std::vector<float> gw((size_t)n_nodes * F), gv(n_nodes), wsq(n_nodes), wv2((size_t)n_nodes * nx);
  for (int c = 0; c < n_nodes; ++c) {
    double sq = 0;
    for (int d = 0; d < F; ++d) gw[(size_t)c * F + d] = (float)w[(size_t)c * F + d];
    for (int d = 0; d < nx; ++d) {
      const double wd = w[(size_t)c * F + 1 + d];
      sq += wd * wd;
      wv2[(size_t)c * nx + d] = (float)(v[c] * wd * wd);
    }
    gv[c] = (float)v[c];
    wsq[c] = (float)sq;
  }
  int rc;
  if ((rc = upload(p, gw, &p->e.gw)) || (rc = upload(p, gv, &p->e.gv)) || (rc = upload(p, wsq, &p->e.gwsq)) ||
      (rc = upload(p, wv2, &p->e.gwv2))) {
    dpi_problem_destroy(p);
    return rc;
  }
  *out = p;
  return 0;
}

int dpi_problem_set_hessian_approximation(dpi_problem p, int sdgd_v) {
  if (!p || sdgd_v < 0 || sdgd_v > 255) return fail(DPI_ERR_ARG, "hessian approximation: 0 <= v <= 255");
  p->e.sdgd_v = sdgd_v;
  return 0;
}

int dpi_problem_set_estimate_delta_t(dpi_problem p, double delta_t) {
  if (!p || !(delta_t >= 0.0) || !(delta_t < 1e30)) return fail(DPI_ERR_ARG, "estimate_delta_t: 0 <= dt < inf");
  p->td_dt = (float)delta_t;
  return 0;
}

int dpi_problem_destroy(dpi_problem p) {
  if (!p) return 0;
  prep_tags_drop(p);
  for (void* d : p->dev) (void)hipFree(d);
  delete p;
  return 0;
}

// The device functor of a problem for the fit's shell entries (dpi_fit.hip, which does not see the handle's
// struct); NULL for a NULL handle.  Host memory of the handle: valid until dpi_problem_destroy.
DPI_HIDDEN const dpi::EqDev* problem_eq(dpi_problem p) { return p ? &p->e : nullptr; }

}  // extern "C"

// PISGradNet pipeline rows (floats per path) and chunking.  x3: split-storage regions, every
// offset a multiple of 32 floats (128 B, one granule-pair chunk); GEMM-output widths (hidden
// units, the nx-wide NO / GX) padded to 64, the IN region to 32.
static PisRows pis_rows_layout(const NetPisDev& pd, bool x3) {
  auto r4 = [](int x) { return (x + 3) & ~3; };
  auto rw = [&](int x) { return x3 ? (x + 63) & ~63 : r4(x); };
  int hmax = 0;
  for (int l = 0; l < pd.L; ++l) hmax = std::max(hmax, pd.h[l]);
  PisRows L;
  int o = 0;
  L.E = o;
  o += 2 * PIS_CH;
  L.T1 = o;
  o += PIS_CH;
  L.IN = o;
  L.INP = x3 ? (PIS_CH + pd.nx + 31) & ~31 : r4(PIS_CH + pd.nx);
  o += L.INP;
  L.H0 = o;
  o += PIS_CH;
  L.H1 = o;
  o += PIS_CH;
  for (int l = 0; l < 4; ++l) {
    L.A[l] = o;
    o += l < pd.L ? rw(pd.h[l]) : 0;
  }
  L.NO = o;
  o += rw(pd.nx);
  L.D0 = o;
  o += rw(hmax);
  L.D1 = o;
  o += rw(hmax);
  L.GX = o;
  o += rw(pd.nx);
  L.SS = o;
  o += rw(pd.nx);
  L.ST = o;
  o += rw(pd.nx);
  L.SC = o;  // s, cI, TD u(t_next), s - t, [split: network time input, smooth]; from PIS_GST the
             // rollout parts' terminal GMM statistics
  o += rw(PIS_GST + PIS_PARTS * NSG);
  L.stride = o;
  return L;
}
// (point, 64-path block) pairs per pipeline chunk.  Default 4096 = 262,144 rows (4 GB of rows
// for PISGradNet 4x512 — HBM is 288 GB): every GEMM of the chain is one launch of 4096
// workgroups, so launch gaps and the last-round tail are amortised.  Measured on HJB configs[2]
// (ms/step): 256 -> 8.57, 512 -> 6.93, 1024 -> 6.41, 4096 -> 6.36.  DPI_PIS_CHUNK overrides.
static int pis_chunk_wg() {
  static const int x = env_int("DPI_PIS_CHUNK", 4096);
  return x >= 1 ? x : 4096;
}

// Workspace: gx[n] | fb[n] | bx[n][H] | hb[n][HBS = 256] | tickets[n] | rec[n][BREC] | ready[n] |
// [PIS rows] | partial[n][nbp][slab_row] | ... | [stash] | [park]  (256-B aligned)
struct WsLayout {
  size_t gx, fb, bx, hb, tk, rec, ready, rows, partial, rq, noise, nq, stash, park, total;
  int rows_cap;
  size_t park_rows;  // rows of the park region (0: none)
};
static size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
// GBM MLP nets stage their noise sums on the prepare stream (dpi_label_prepare -> k_noise_shared;
// DPI_GBM_PREP=0 disables it): the workspace then holds them, [n][nbp][2][4 nb][P] floats.
static bool gbm_noise_prep(dpi_problem p, dpi_net net) {
  static const bool on = env_int("DPI_GBM_PREP", 1) != 0;
  return on && p && net && net->d.kind == 1 && p->e.kind == DPI_EQ_GBM;
}
// the pairs for which dpi_label_prepare stages anything (the others' fused path kernels do it all)
static bool stages_prepare(dpi_problem p, dpi_net net) {
  return (net->d.kind == 2 || gbm_noise_prep(p, net)) && !(p->td_dt > 0.f);
}
// park: the pair's workspace holds the park (Route::park): DPI_PARK_MAX_BLOCKS rows of PARK_ROW floats,
// one per path block of a call, in which a terminal-first block keeps its terminal sums across the
// MLP (dpi_device.h paths_body).  A constant, so the workspace stays affine in n and M; a call with
// more path blocks than rows leaves it unused and runs every block terminal-last.
static bool park_pair(dpi_problem p, dpi_net net);
// The optional regions a layout is asked for, by name: ws_layout(.., {.park = r.park}); {}: neither.
struct WsRegions {
  bool noise = false, park = false;
};
static WsLayout ws_layout(dpi_net net, int n, int M, int F, WsRegions want) {
  WsLayout w;
  // bx rows: the specialised image's H, or the general one's width cap (the wider of the two)
  const int H = (net && net->d.kind == 1) ? std::max(net->spec ? net->d.H : 0, net->gen ? net->g.H : 0) : 0;
  const size_t nbp = (size_t)(M + P - 1) / P;
  w.gx = 0;
  w.fb = al256((size_t)n * 4);
  w.bx = w.fb + al256((size_t)n * 4);
  w.hb = w.bx + al256((size_t)n * H * 4);
  w.tk = w.hb + al256((size_t)n * HBS * 4);  // the fused reduce's per-point tickets (k_paths)
  // the one-launch dpi_sample_with_gradients' per-point baseline records and hand-off words
  w.rec = w.tk + al256((size_t)n * 4);
  w.ready = w.rec + al256((size_t)n * BREC * 4);
  w.rows = w.ready + al256((size_t)n * 8);
  w.rows_cap = 0;
  size_t rows_bytes = 0;
  if (net && net->d.kind == 2) {
    // a chunk of path rows plus the n per-point baseline rows, which ride in the first chunk's chain
    w.rows_cap = (int)std::min((size_t)n * nbp * P, (size_t)pis_chunk_wg() * P) + n;
    const int stride = std::max(pis_rows_layout(net->pis, false).stride, pis_rows_layout(net->pis, true).stride);
    rows_bytes = al256((size_t)w.rows_cap * stride * 4);
  }
  w.partial = w.rows + rows_bytes;
  w.rq = w.partial + al256((size_t)n * nbp * slab_row(F) * 4);
  // PISGradNet: the shared rollout's queue counter (256 B) and per-SIMD claim words
  w.noise = w.rq + ((net && net->d.kind == 2) ? 256 + (size_t)PIS_CLAIM_SLOTS * 4 : 0);
  const size_t nb4 = (size_t)((F - 1 + 3) / 4) * 4;
  w.nq = w.noise + (want.noise ? al256((size_t)n * nbp * 2 * nb4 * P * 4) : 0);
  // k_noise_shared's queue counter (256 B) and per-SIMD claim words
  w.total = w.nq + (want.noise ? 256 + (size_t)PIS_CLAIM_SLOTS * 4 : 0);
  // the general MLP family's stash (dpi_general.h): one slot per workgroup of its path launch, a fixed
  // count — it does not grow with n or M.  The last region, so every other offset stays where it was.
  // A gradient-head net parks nothing: no stash region.
  w.stash = w.total;
  if (net && net->d.kind == 1 && net->gen && !net->head) {
    w.stash = al256(w.total);
    w.total = w.stash + al256((size_t)gen_slots(net->g.H) * gen_slot_floats(net->g.L, net->g.ht) * 4);
  }
  // the park: the last region again, so every other offset stays where it was
  w.park = w.total;
  w.park_rows = 0;
  if (want.park) {
    w.park_rows = (size_t)DPI_PARK_MAX_BLOCKS;
    w.park = al256(w.total);
    w.total = w.park + w.park_rows * PARK_ROW * 4;
  }
  return w;
}

// GEMM precision (include/dpi.h DPI_GEMM_*): AUTO (default) and F16X3 run the fp16-split MFMA
// everywhere — the fused MLP of k_paths and the PISGradNet pipeline in split storage
// (k_gemm_x3); F32 runs exact-fp32 MFMA (mlp_tile, k_gemm_nt) for ablation.  DPI_GEMM=f32|f16x3
// sets the initial mode.
static int g_gemm_mode = -1;  // -1: from the environment
static int gemm_mode() {
  if (g_gemm_mode < 0) {
    const char* e = std::getenv("DPI_GEMM");
    g_gemm_mode = !e ? DPI_GEMM_AUTO : std::strcmp(e, "f16x3") == 0 ? DPI_GEMM_F16X3
                                   : std::strcmp(e, "f32") == 0   ? DPI_GEMM_F32
                                                                  : DPI_GEMM_AUTO;
  }
  return g_gemm_mode;
}
static int net_mode(dpi_net net) { return (net && net->precision >= 0) ? net->precision : gemm_mode(); }
static bool mlp_split(dpi_net net) { return net_mode(net) != DPI_GEMM_F32; }
static bool pis_x3(dpi_net net) { return net_mode(net) != DPI_GEMM_F32; }
static int* net_status(dpi_net net) {
  return (net && net->finite && net->status) ? net->status + (size_t)net->slot * STATUS_STRIDE : nullptr;
}

extern "C" int dpi_set_gemm_precision(int mode) {
  if (mode != DPI_GEMM_F32 && mode != DPI_GEMM_F16X3 && mode != DPI_GEMM_AUTO)
    return fail(DPI_ERR_ARG, "gemm precision: 0 = fp32, 1 = fp16-split, 2 = auto");
  g_gemm_mode = mode;
  return 0;
}

// The GEMM launches' run-time epilogue as the kernels' EPI_* template constant: f(integral_constant).
template <class F>
static void with_epi(int epi, F f) {
  if (epi == EPI_BIAS)
    f(std::integral_constant<int, EPI_BIAS>{});
  else if (epi == EPI_BIAS_ELU)
    f(std::integral_constant<int, EPI_BIAS_ELU>{});
  else
    f(std::integral_constant<int, EPI_DELU>{});
}

static void gemm(int epi, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 const float* bias, const float* aux, int ldaux, hipStream_t st) {
  dim3 grid((M + GBM_ - 1) / GBM_, (N + GBN_ - 1) / GBN_), block(256);
  with_epi(epi, [&](auto e) {
    hipLaunchKernelGGL(k_gemm_nt<decltype(e)::value>, grid, block, 0, st, M, N, K, A, lda, B, ldb, C, ldc, bias, aux,
                       ldaux);
  });
}

static int cu_count() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    ncu = std::max(1, ncu);
  }
  return ncu;
}

// DELU epilogue operands staged through the ring's last two DMA slots (k_gemm_x3); DPI_X3_STAGE=0
// loads them in the epilogue instead (ablation).
static int x3_stage_aux() {
  static const int v = env_int("DPI_X3_STAGE", 1) != 0;
  return v;
}

// Block tile of the NT = 4 split GEMMs: 128 (default, k_gemm_x3h: two blocks per CU) or 256
// (DPI_X3_TILE=256: k_gemm_x3, one 8-wave block per CU with the staged DELU epilogue).
static int x3_tile_rows() {
  static const int v = env_int("DPI_X3_TILE", 128) == 256 ? 256 : 128;
  return v;
}

// Split-storage GEMM: OUT (M x Np) = epi(X (M x Kp) W^T), all split (Np, Kp multiples of 32).
template <int NT>
static void gemm_x3_nt(int epi, int M, int Kp, int Np, const uint32_t* W, float ws, const float* X, int ldx,
                       const float* X2, int ldx2, int k1, float* OUT, int ldc, const float* bias, const float* aux,
                       int ldaux, float os, float as, hipStream_t st) {
  const int nnt = Np / (32 * NT), nmt = (M + X3_BM - 1) / X3_BM, nk1 = k1 / 32;
  if constexpr (NT == 4) {
    if (x3_tile_rows() == 128) {
      const int nmh = (M + X3H_BM - 1) / X3H_BM;
      dim3 gh(nnt * nmh), bh(X3H_THREADS);
      with_epi(epi, [&](auto e) {
        hipLaunchKernelGGL(k_gemm_x3h<decltype(e)::value>, gh, bh, 0, st, M, Kp, nnt, W, ws, X, ldx, X2, ldx2, nk1, OUT,
                           ldc, bias, aux, ldaux, os, as);
      });
      return;
    }
  }
  dim3 grid(nnt * nmt), block(X3_THREADS);
  with_epi(epi, [&](auto e) {  // only the DELU epilogue has operands to stage
    constexpr int E = decltype(e)::value;
    hipLaunchKernelGGL((k_gemm_x3<E, NT>), grid, block, 0, st, M, Kp, nnt, W, ws, X, ldx, X2, ldx2, nk1, OUT, ldc, bias,
                       aux, ldaux, os, as, E == EPI_DELU ? x3_stage_aux() : 0);
  });
}
// ws: the weight matrix's scale 2^-s (pack_split_x3) with the operand exponents folded in; os / as:
// the ELU output's store scale / the DELU operand's read scale (dpi_gemm.h).  X2 != nullptr: K
// columns [k1, Kp) come from X2.
static void gemm_x3(int epi, int M, int Kp, int Np, const uint32_t* W, float ws, const float* X, int ldx, float* OUT,
                    int ldc, const float* bias, const float* aux, int ldaux, float os, float as, hipStream_t st,
                    const float* X2 = nullptr, int ldx2 = 0, int k1 = 0) {  // Np % 64 == 0, Kp % 32 == 0
  if (!X2) X2 = X, ldx2 = ldx, k1 = Kp;
  if (Np % 128 == 0)
    gemm_x3_nt<4>(epi, M, Kp, Np, W, ws, X, ldx, X2, ldx2, k1, OUT, ldc, bias, aux, ldaux, os, as, st);
  else
    gemm_x3_nt<2>(epi, M, Kp, Np, W, ws, X, ldx, X2, ldx2, k1, OUT, ldc, bias, aux, ldaux, os, as, st);
}

// k_pis_net (the fused split VJP chain) by default; DPI_PIS_FUSED=0 selects the layer-wise
// k_gemm_x3h chain (read per call, so one process can compare both).
static bool pis_fused_on() { return env_int("DPI_PIS_FUSED", 1) != 0; }
// k_pis_net's shapes: 1-4 hidden layers of 512 units, nx <= 128 (X in <= 4 chunks, GX 64 or 128 wide)
static bool pis_fused_fits(const NetPisDev& pd, const PisRows& L) {
  if (pd.L < 1 || pd.L > 4) return false;
  for (int l = 0; l < pd.L; ++l)
    if (pd.h[l] != PN_H) return false;
  const int nxk = L.INP / 32 - 2, nop = (pd.nx + 63) & ~63;
  return nxk >= 1 && nxk <= PN_XC && (nop == 64 || nop == 128);
}

// The PISGradNet chain of pis_chain in split storage (every width padded to 32; the x part of IN
// starts at its chunk 2 = word 64).
static PisRows pis_chain_x3(const NetPisDev& pd, float* rows, int R, hipStream_t st, bool vjp = true) {
  PisRows L = pis_rows_layout(pd, true);
  auto r64 = [](int x) { return (x + 63) & ~63; };
  const int ld = L.stride, NXK = (pd.nx + 31) & ~31, NOP = r64(pd.nx);
  // t_encoder -> IN[:, 0:64] and smooth -> SC + 5 in one launch (one block per CU: 144 KB of weights in LDS)
  if (R > 0) {
    const int ncu = cu_count();
    const int blocks = std::max(1, std::min(ncu, (R + 16 * (PT_THREADS / 64) - 1) / (16 * (PT_THREADS / 64))));
    hipLaunchKernelGGL(k_pis_time<4>, dim3(blocks), dim3(PT_THREADS), 0, st, pd, rows, L, R);
  }
  // the VJP chain as one launch with the activations in LDS (dpi_pisnet.h), where the shape fits
  if (vjp && R > 0 && pis_fused_on() && pis_fused_fits(pd, L)) {
    const dim3 grid((R + PN_BM - 1) / PN_BM), block(PN_THREADS);
    // row loads non-temporal, stores plain (k_pis_net's NTM = 1)
    hipEvent_t t0, t1;
    take_timer(t0, t1);
    auto launch = [&](auto nlc) {
      hipExtLaunchKernelGGL((k_pis_net<1, decltype(nlc)::value>), grid, block, 0, st, t0, t1, 0, pd, rows, L, R);
    };
    switch (pd.L) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      default: launch(std::integral_constant<int, 4>{}); break;
    }
    return L;
  }
  int Kp = L.INP;
  const float* a = rows + L.IN;
  for (int l = 0; l < pd.L; ++l) {
    const int Np = r64(pd.h[l]);
    gemm_x3(EPI_BIAS_ELU, R, Kp, Np, pd.nnS[l], pd.nnW[l], a, ld, rows + L.A[l], ld, pd.nnbP[l], nullptr, 0, pd.nnO[l],
            1.0f, st);
    a = rows + L.A[l];
    Kp = Np;
  }
  if (!vjp) {  // forward only (TD terminal value): net_out
    gemm_x3(EPI_BIAS, R, Kp, NOP, pd.nnS[pd.L], pd.nnW[pd.L], a, ld, rows + L.NO, ld, pd.nnbP[pd.L], nullptr, 0, 1.0f, 1.0f,
            st);
    return L;
  }
  // VJP: the x part of IN starts at its chunk 2 (word 64).  (Fusing this product into the last
  // forward layer's launch, elu' read back from the tile the block had just stored, measured no
  // faster: 828 us against 487 + 335 us.)
  int dcur = L.D0, dnext = L.D1;
  gemm_x3(EPI_DELU, R, NXK, r64(pd.h[pd.L - 1]), pd.nnTS[pd.L], pd.nnTW[pd.L], rows + L.IN + 2 * 32, ld, rows + dcur, ld,
          nullptr, rows + L.A[pd.L - 1], ld, 1.0f, pd.nnA[pd.L - 1], st);
  for (int l = pd.L - 1; l >= 1; --l) {
    gemm_x3(EPI_DELU, R, r64(pd.h[l]), r64(pd.h[l - 1]), pd.nnTS[l], pd.nnTW[l], rows + dcur, ld, rows + dnext, ld, nullptr,
            rows + L.A[l - 1], ld, 1.0f, pd.nnA[l - 1], st);
    std::swap(dcur, dnext);
  }
  // GX = net_out + J^T X = [A_{L-1} | D_0] . [nn[L] | nnT[0]]^T + b_L: one GEMM with K = h_{L-1} + h_0,
  // the A_{L-1} chunks first (k_pis_net's order; k_pis_final and k_pis_base_final only need the sum)
  gemm_x3(EPI_BIAS, R, Kp + r64(pd.h[0]), NOP, pd.gxnoS, pd.gxnoW, rows + L.A[pd.L - 1], ld, rows + L.GX, ld,
          pd.nnbP[pd.L], nullptr, 0, 1.0f, 1.0f, st, rows + dcur, ld, Kp);
  return L;
}

// PISGradNet forward + VJP over R rows (solution.py:256-289); returns the row layout with H0 pointing
// at the last smooth_net activation.
static PisRows pis_chain(const NetPisDev& pd, float* rows, int R, hipStream_t st, bool vjp = true) {
  PisRows L = pis_rows_layout(pd, false);
  const int ld = L.stride, C = PIS_CH, nx = pd.nx;
  // t_encoder -> IN[:, 0:64]
  gemm(EPI_BIAS_ELU, R, C, 2 * C, rows + L.E, ld, pd.te0, 2 * C, rows + L.T1, ld, pd.te0b, nullptr, 0, st);
  gemm(EPI_BIAS, R, C, C, rows + L.T1, ld, pd.te2, C, rows + L.IN, ld, pd.te2b, nullptr, 0, st);
  // smooth_net hidden activations (elu applied on store: each is consumed through an ELU)
  int hs = L.H0, ho = L.H1;
  gemm(EPI_BIAS_ELU, R, C, 2 * C, rows + L.E, ld, pd.sn0, 2 * C, rows + hs, ld, pd.sn0b, nullptr, 0, st);
  for (int j = 0; j < pd.nsm; ++j) {
    gemm(EPI_BIAS_ELU, R, C, C, rows + hs, ld, pd.sn[j], C, rows + ho, ld, pd.snb[j], nullptr, 0, st);
    std::swap(hs, ho);
  }
  // nn_module forward
  int in = C + nx;
  const float* a = rows + L.IN;
  for (int l = 0; l < pd.L; ++l) {
    gemm(EPI_BIAS_ELU, R, pd.h[l], in, a, ld, pd.nn[l], in, rows + L.A[l], ld, pd.nnb[l], nullptr, 0, st);
    a = rows + L.A[l];
    in = pd.h[l];
  }
  gemm(EPI_BIAS, R, nx, in, a, ld, pd.nn[pd.L], in, rows + L.NO, ld, pd.nnb[pd.L], nullptr, 0, st);
  L.H0 = hs;
  if (!vjp) return L;
  // VJP with cotangent X on net_out: D_{L-1} = (X nn_L) * elu'(A_{L-1}), ..., GX = D_0 nn_0[:, 64:]
  int dcur = L.D0, dnext = L.D1;
  gemm(EPI_DELU, R, pd.h[pd.L - 1], nx, rows + L.IN + PIS_IN_OFF, ld, pd.nnT[pd.L], nx, rows + dcur, ld, nullptr,
       rows + L.A[pd.L - 1], ld, st);
  for (int l = pd.L - 1; l >= 1; --l) {
    gemm(EPI_DELU, R, pd.h[l - 1], pd.h[l], rows + dcur, ld, pd.nnT[l], pd.h[l], rows + dnext, ld, nullptr,
         rows + L.A[l - 1], ld, st);
    std::swap(dcur, dnext);
  }
  gemm(EPI_BIAS, R, nx, pd.h[0], rows + dcur, ld, pd.nnT[0], pd.h[0], rows + L.GX, ld, nullptr, nullptr, 0, st);
  L.H0 = hs;
  return L;
}

extern "C" size_t dpi_workspace_bytes(dpi_problem p, dpi_net net, int n, int M) {
  if (!p || n < 0 || M < 0) return 0;
  return ws_layout(net, n, M, 1 + p->e.nx, {.park = park_pair(p, net)}).total;
}
// + the staged noise sums of a GBM MLP net's prepared calls (the last region of the layout, so a
// plain call's offsets are the same)
extern "C" size_t dpi_workspace_bytes_prepared(dpi_problem p, dpi_net net, int n, int M) {
  if (!p || n < 0 || M < 0) return 0;
  return ws_layout(net, n, M, 1 + p->e.nx, {.noise = gbm_noise_prep(p, net), .park = park_pair(p, net)}).total;
}

// the counters of draws 1-3 (k_sample_points, k_baseline's in-block sampling)
static SampleSpec sample_spec(dpi_problem p, uint64_t seed, uint32_t epoch, uint32_t point_base, float eps,
                              int t_factors, float* tx) {
  SampleSpec s;
  s.tx = tx;
  s.k0 = (uint32_t)seed;
  s.k1 = (uint32_t)(seed >> 32);
  s.c3t = DPI_TAG_T | (epoch << 8);
  s.c3x0 = DPI_TAG_X0 | (epoch << 8);
  s.c3x = DPI_TAG_X | (epoch << 8);
  s.point_base = point_base;
  s.eps = eps;
  s.alpha_init_sqrt = p->alpha_init_sqrt;
  s.t_factors = t_factors;
  return s;
}

extern "C" int dpi_sample_points(dpi_problem p, int n, uint64_t seed, uint32_t epoch, uint32_t point_base, float eps,
                      float* tx, void* stream) {
  return dpi_sample_points_t(p, n, seed, epoch, point_base, eps, 0, tx, stream);
}

extern "C" int dpi_sample_points_t(dpi_problem p, int n, uint64_t seed, uint32_t epoch, uint32_t point_base, float eps,
                                   int t_factors, float* tx, void* stream) {
  if (!p || (!tx && n) || n < 0 || epoch > 0xFFFFFFu || t_factors < 0 || t_factors > 4096)
    return fail(DPI_ERR_ARG, "sample_points: bad arguments (t_factors in [0, 4096])");
  if (n == 0) return 0;
  const int nb = (p->e.nx + 3) >> 2;
  const int total = n * nb;
  const SampleSpec s = sample_spec(p, seed, epoch, point_base, eps, t_factors, tx);
  dim3 grid((total + 255) / 256), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (p->e.kind) {
    case DPI_EQ_CHA:
      hipLaunchKernelGGL(k_sample_points<DPI_EQ_CHA>, grid, block, 0, st, p->e, n, s);
      break;
    case DPI_EQ_OU:
      hipLaunchKernelGGL(k_sample_points<DPI_EQ_OU>, grid, block, 0, st, p->e, n, s);
      break;
    case DPI_EQ_GBM:
      hipLaunchKernelGGL(k_sample_points<DPI_EQ_GBM>, grid, block, 0, st, p->e, n, s);
      break;
    default:
      return fail(DPI_ERR_UNSUPPORTED, "sample_points: equation kind");
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The route of a pair for one kind of call (dpi_route.h), in the net's effective GEMM mode.
static Route pair_route(dpi_problem p, dpi_net net, RouteCall call) {
  return route(route_pair(p, net, p->td_dt > 0.f, mlp_split(net)), call);
}
static int refuse(const Route& r) { return fail(r.code, std::string(r.pre) + r.msg); }
// ... behind the null check of every entry point; refuses what is due before the call's own arguments
// are looked at (a late refusal stays in *r: label_args returns it once they have passed).
static int route_call(dpi_problem p, dpi_net net, RouteCall call, Route* r) {
  if (!p || !net) return fail(DPI_ERR_ARG, "null problem or net");
  *r = pair_route(p, net, call);
  return r->code && r->stage != ROUTE_LATE ? refuse(*r) : 0;
}
static bool park_pair(dpi_problem p, dpi_net net) { return p && net && pair_route(p, net, ROUTE_PATHS).park; }

// One label call as its entry point received it: the dpi_label_*, dpi_generate_* and
// dpi_sample_with_gradients entry points fill it once, field by field, and the host side passes it on
// whole.  What follows from it alone is computed here and nowhere else.
struct LabelCall {
  dpi_problem p = nullptr;
  dpi_net net = nullptr;
  const float* tx = nullptr;
  int n = 0, M = 0, K = 0;
  uint64_t seed = 0;
  uint32_t epoch = 0, point_base = 0;
  int m_begin = 0, m_end = 0, flags = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stream = nullptr;
  // the outputs the entry point has: the sums, and the finalized labels y clipped at bound
  float *moments = nullptr, *hessian_sums = nullptr, *y = nullptr;
  float bound = 0.f;
  // the kind of entry point: the route it asks for; dpi_label_prepare stages only (it has no outputs)
  RouteCall call = ROUTE_PATHS;
  bool stage_only = false;
  bool hess() const { return call == ROUTE_HESS; }
  bool prepared() const { return stage_only || (flags & DPI_PREPARED); }  // dpi_label_prepare, or the call it feeds
  bool noise() const { return prepared() && gbm_noise_prep(p, net); }    // ... with the noise staging region
  // floats per row of y: the first-order labels, then the Hessian's
  int ystride() const { return 1 + p->e.nx + (hess() ? p->e.nx * p->e.nx : 0); }
  char* base() const { return (char*)ws; }
  hipStream_t st() const { return (hipStream_t)stream; }
};

// ---- the workspace tag: what the host knows of a workspace, one record per pointer under one mutex.
// base_n: the fused reduce (k_paths' last block per point) counts blocks on per-point tickets that the
// baseline launch zeroes and the last block resets.  The tag holds the point count of the baseline
// enqueued on the workspace, and a fused label call on a workspace without one fails instead of running
// a reduce whose tickets hold garbage (it would never fire and leave the labels unwritten).
// prep, the DPI_PREPARED contract: a prepared label call trusts that dpi_label_prepare staged the first
// chunk in the same workspace with the same arguments.  dpi_label_prepare records them (host side: no
// device read, no sync); the prepared call must match them and consumes the record, so a mismatched or
// repeated call fails with DPI_ERR_ARG instead of producing labels from another batch's rollout.  The
// GEMM mode is among them (split and fp32 rows differ in layout): a precision switch between prepare and
// the prepared call fails instead of reading rows laid out the other way.
struct PrepTag {
  const void *p, *net, *tx;
  int n, M, K, m_begin, m_end, flags, mode;
  uint64_t seed;
  uint32_t epoch, point_base;
  size_t ws_bytes;
  bool operator==(const PrepTag& o) const {
    return p == o.p && net == o.net && tx == o.tx && n == o.n && M == o.M && K == o.K && m_begin == o.m_begin &&
           m_end == o.m_end && flags == o.flags && mode == o.mode && seed == o.seed && epoch == o.epoch &&
           point_base == o.point_base && ws_bytes == o.ws_bytes;
  }
};
static PrepTag prep_tag(const LabelCall& c) {
  return PrepTag{.p = c.p, .net = c.net, .tx = c.tx, .n = c.n, .M = c.M, .K = c.K, .m_begin = c.m_begin,
                 .m_end = c.m_end, .flags = c.flags & DPI_BOTH, .mode = pis_x3(c.net) ? 1 : 0, .seed = c.seed,
                 .epoch = c.epoch, .point_base = c.point_base, .ws_bytes = c.ws_bytes};
}
struct WsTag {
  int base_n = 0;               // points of the baseline enqueued on the workspace (0: none)
  std::optional<PrepTag> prep;  // dpi_label_prepare's record, until a label call consumes or invalidates it
};
static std::mutex g_ws_mu;
static std::unordered_map<const void*, WsTag>& ws_tags() {
  static std::unordered_map<const void*, WsTag> m;
  return m;
}
static void base_tag_set(const void* ws, int n) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  ws_tags()[ws].base_n = n;
}
static bool base_tag_ok(const void* ws, int n) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  auto it = ws_tags().find(ws);
  return it != ws_tags().end() && it->second.base_n == n;
}
static void prep_tag_set(const LabelCall& c) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  ws_tags()[c.ws].prep = prep_tag(c);
}
// The workspace's prepare record, and the record gone.
static std::optional<PrepTag> prep_tag_take(const void* ws) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  auto it = ws_tags().find(ws);
  return it == ws_tags().end() ? std::nullopt : std::exchange(it->second.prep, std::nullopt);
}
void prep_tags_drop(const void* owner) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  for (auto& kv : ws_tags())
    if (kv.second.prep && (kv.second.prep->p == owner || kv.second.prep->net == owner)) kv.second.prep.reset();
}
extern "C" int dpi_workspace_forget(const void* ws, size_t ws_bytes) {
  const char *lo = (const char*)ws, *hi = lo + ws_bytes;
  std::lock_guard<std::mutex> g(g_ws_mu);
  for (auto it = ws_tags().begin(); it != ws_tags().end();)
    it = ((const char*)it->first >= lo && (const char*)it->first < hi) ? ws_tags().erase(it) : std::next(it);
  return 0;
}

// The launch of the route's unit.  A unit that cannot serve the call it was chosen for is a bug in the
// route: reported here, for every entry point.
static int launch_unit(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  if (q.unit < N_UNITS && UNIT_FNS[q.unit](p, net, q)) return 0;
  return fail(DPI_ERR_UNSUPPORTED, std::string("internal error: the route chose a unit that holds no kernel for the call (") +
                                       (q.unit < N_UNITS ? UNIT_NAMES[q.unit] : "none") + ")");
}

// The two kinds of Launch.  The per-point baseline of n points writes the workspace's gx / fb / bx /
// hb regions and zeroes the fused reduce's tickets; a path launch (k_paths, k_paths_fb) runs nblocks
// workgroups over a's paths.
static Launch baseline_launch(const Route& r, const float* tx, int n, void* ws, const WsLayout& w, hipStream_t st) {
  char* b = (char*)ws;
  Launch q;
  q.unit = r.unit;
  q.baseline = true;
  q.tx = tx;
  q.n = n;
  q.gx = (float*)(b + w.gx);
  q.fb = (float*)(b + w.fb);
  q.bx = (float*)(b + w.bx);
  q.hb = (float*)(b + w.hb);
  q.tickets = (int*)(b + w.tk);
  q.st = st;
  return q;
}
static Launch path_launch(const Route& r, const PathArgs& a, int nblocks, const LabelCall& c, const WsLayout& w) {
  Launch q;
  q.unit = r.unit;
  q.a = &a;
  q.nblocks = nblocks;
  q.st = c.st();
  if (r.stash) q.stash = (floatx4*)(c.base() + w.stash);
  return q;
}

extern "C" {
// The family question alone (ROUTE_FAMILY), with the caller's td.
int dpi_pair_family(dpi_problem p, dpi_net net, int td, int* family) {
  if (!p || !net || !family) return fail(DPI_ERR_ARG, "pair_family: null problem, net or family");
  const Route r = route(route_pair(p, net, td != 0, mlp_split(net)), ROUTE_FAMILY);
  *family = r.family;
  if (r.code) return refuse(r);
  if (net->d.kind == 1 && !r.general && !spec_shape(p->e.kind, net->d.H, net->d.L))
    return fail(DPI_ERR_UNSUPPORTED, "pair_family: unsupported equation/network shape");
  return 0;
}

int dpi_general_slots(dpi_net net, int* slots) {
  if (!net || !slots) return fail(DPI_ERR_ARG, "general_slots: null net or slots");
  *slots = (net->d.kind == 1 && net->gen && !net->head) ? gen_slots(net->g.H) : 0;
  return 0;
}

static int pis_check(dpi_problem p) {
  if (p->e.kind != DPI_EQ_OU)
    return fail(DPI_ERR_UNSUPPORTED, "PISGradNet device net needs OUProcessEquation (its g0 is the problem's GMM g)");
  return 0;
}

// PISGradNet: nothing to launch.  The per-point f_b = f(t, x, u, grad u) needs the whole
// PISGradNet chain, so its n rows ride in the first path chunk's chain, and g(x) is formed beside it
// in k_pis_base_final (pis_paths): every label call computes both before k_pis_final and the reduce
// read them, and the prepare stream's rollout needs neither.
static int pis_baseline(dpi_problem p) { return pis_check(p); }

// Independent Philox chains per wave in the PISGradNet rollout: 4 (default; 61 VGPRs) or 2
// (DPI_PIS_UNROLL=2; 47 VGPRs, room beside the 256 x 128 GEMM's blocks).
static int pis_rollout_unroll() {
  static const int v = env_int("DPI_PIS_UNROLL", 4) == 2 ? 2 : 4;
  return v;
}

// The prepare stream's rollout as the per-SIMD-capped work queue (k_pis_rollout_shared), launched
// with DPI_PIS_PREP_SHARED (default 2) waves per SIMD more than it keeps; 0: the plain grid.
static int pis_prep_shared() {
  static const int v = env_int("DPI_PIS_PREP_SHARED", 2, 0, 8);
  return v;
}

// Path sets of a prepared chunk the prepare stream rolls out: DPI_PIS_PREP_FRAC (default 0.92) of
// them; the shared rollout beside k_pis_net runs at about a third of its stand-alone rate, so the
// rest goes to the prepared call's head at full occupancy (r04f trace: the prepare-stream rollout
// of the whole chunk, 4.07 ms, outlasted the 3.75 ms chain it hid under).  Round 6 sweeps on two
// boxes (profiles/r06x, r06y; 60 steps, two runs each): f = 0.88 3.738 / 3.752 and 3.798 / 3.806
// ms/step against 0.92's 3.763 / 3.774 and 3.831 / 3.827 (0.82: 3.797 / 3.810; 0.96, 1.0, 0.76 slower).
static int pis_prep_sets(int g) {
  static const double f = env_real("DPI_PIS_PREP_FRAC", 0.88, 0.0, 1.0);
  return std::max(0, std::min(g, (int)(f * g + 0.5)));
}

// prepared: dpi_label_prepare already ran the first chunk's rollout and baseline rows (same
// arguments, same workspace); prepare_only: run just those (dpi_label_prepare).
static int pis_paths(const LabelCall& c, const PathArgs& a, const WsLayout& w) {
  const dpi_problem p = c.p;
  const dpi_net net = c.net;
  const float* tx = c.tx;
  const int n = c.n, K = c.K;
  char* b = c.base();
  hipStream_t st = c.st();
  const bool prepare_only = c.stage_only, prepared = !prepare_only && c.prepared();
  int rc = pis_check(p);
  if (rc) return rc;
  float* rows = (float*)(b + w.rows);
  float* fb = (float*)(b + w.fb);
  const bool x3 = pis_x3(net);
  const PisRows L = pis_rows_layout(net->pis, x3);
  const int G = n * a.nbp, GC = std::max(1, (w.rows_cap - n) / P);
  const float dt = a.td_dt;
  // TD estimators: a terminal stage (rollout to t_next, forward chain, a_p = u(t_next, X) - g(x))
  // before the integral stage; the plain estimators run both paths in one rollout.
  // The first chunk's integral chain also carries the n baseline rows (t_i, x_i) after its g P path
  // rows: f_b comes out of the same GEMM launches (row results do not depend on where a row sits in
  // the chunk) and lands before k_pis_final reads it.
  auto chunk = [&](auto x3c, int g0, int g) {
    constexpr bool X3 = decltype(x3c)::value;
    auto chain = [&](bool vjp, int R) {
      return X3 ? pis_chain_x3(net->pis, rows, R, st, vjp) : pis_chain(net->pis, rows, R, st, vjp);
    };
    // path sets [0, gprep) of a prepared first chunk roll out on the prepare stream (beside the
    // previous batch's chain), the rest [gprep, g) at full occupancy at the head of the prepared
    // call, so the two streams' critical paths balance (DPI_PIS_PREP_FRAC)
    const int gprep = (prepare_only || prepared) ? pis_prep_sets(g) : g;
    auto rollout = [&](int stage, int gbeg = 0) {
      if constexpr (X3) {  // (k_pis_net, which it hides under, exists for the split rows only)
        if (prepare_only && pis_prep_shared()) {
          // the prepare stream: at most one rollout wave per SIMD beside the previous batch's chain
          int* rq = (int*)(b + w.rq);
          (void)hipMemsetAsync(rq, 0, 256 + (size_t)PIS_CLAIM_SLOTS * 4, st);
          hipLaunchKernelGGL((k_pis_rollout_shared<DPI_EQ_OU, true>), dim3(4 * cu_count() * (1 + pis_prep_shared())),
                             dim3(P), 0, st, p->e, net->pis, tx, g0, a.nbp, a.m_begin, K, a.flags, a.k0, a.k1, a.c3t,
                             a.c3s, a.c3i, a.point_base, rows, L, stage, dt, 0, 2 * PIS_PARTS * gprep, rq, rq + 64,
                             1);
          return;
        }
      }
      const int gend = prepare_only ? gprep : g;
      if (gend <= gbeg) return;
      // two one-wave blocks (terminal, integral) per path set of [gbeg, gend): (path, dim part) tasks
      const dim3 grid(2 * PIS_PARTS * (gend - gbeg)), block(P);
      auto launch = [&](auto unr) {
        hipLaunchKernelGGL((k_pis_rollout<DPI_EQ_OU, X3, decltype(unr)::value>), grid, block, 0, st, p->e, net->pis, tx,
                           g0, a.nbp, a.m_begin, K, a.flags, a.k0, a.k1, a.c3t, a.c3s, a.c3i, a.point_base, rows, L,
                           stage, dt, gbeg);
      };
      if (pis_rollout_unroll() == 4)
        launch(std::integral_constant<int, 4>{});
      else
        launch(std::integral_constant<int, 2>{});
    };
    const bool base = g0 == 0;
    float* brows = rows + (size_t)g * P * L.stride;
    if (dt > 0.f) {
      rollout(PIS_TD_TERM);
      if (a.flags & DPI_TERMINAL) {
        const PisRows Lt = chain(false, g * P);
        hipLaunchKernelGGL((k_pis_tvalue<DPI_EQ_OU, X3>), dim3(g), dim3(256), 0, st, p->e, net->pis, tx, g0, a.nbp,
                           rows, Lt, g * P, dt);
      }
      rollout(PIS_TD_INT);
    } else if (!(prepared && base)) {
      rollout(PIS_BOTH);
    } else if (gprep < g) {
      rollout(PIS_BOTH, gprep);  // the prepared chunk's remaining path sets
    }
    if (base && !(prepared && dt == 0.f))
      hipLaunchKernelGGL(k_pis_points<X3>, dim3(n), dim3(64), 0, st, p->e.nx, net->pis, tx, n, brows, L);
    if (prepare_only) return;
    const PisRows Lc = chain(true, g * P + (base ? n : 0));
    if (base)
      hipLaunchKernelGGL((k_pis_base_final<DPI_EQ_OU, X3>), dim3((n + 63) / 64), dim3(256), 0, st, p->e, net->pis,
                         tx, brows, Lc, n, fb, (float*)(b + w.gx));
    hipLaunchKernelGGL((k_pis_final<DPI_EQ_OU, X3>), dim3(g), dim3(NTH), 0, st, p->e, net->pis, tx, g0, a.nbp,
                       a.m_begin, a.m_end, K, a.flags, fb, a.gx, rows, Lc, a.partial, dt);
  };
  for (int g0 = 0; g0 < G; g0 += GC) {
    const int g = std::min(GC, G - g0);
    if (x3)
      chunk(std::true_type{}, g0, g);
    else
      chunk(std::false_type{}, g0, g);
    if (prepare_only) break;  // the first chunk only
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_point_baseline(dpi_problem p, dpi_net net, const float* tx, int n, void* ws, size_t ws_bytes, void* stream) {
  Route r;
  int rc = route_call(p, net, ROUTE_BASELINE, &r);
  if (rc) return rc;
  if (n < 0 || (n && (!tx || !ws))) return fail(DPI_ERR_ARG, "point_baseline: bad arguments");
  if (n == 0) return 0;
  const WsLayout w = ws_layout(net, n, 0, 1 + p->e.nx, {});
  if (ws_bytes < w.partial) return fail(DPI_ERR_WORKSPACE, "workspace too small");
  if (net->d.kind == 2) return pis_baseline(p);
  if ((rc = launch_unit(p, net, baseline_launch(r, tx, n, ws, w, (hipStream_t)stream)))) return rc;
  HIPCHK(hipGetLastError());
  base_tag_set(ws, n);
  return 0;
}

// The label reduce inside k_paths (fused_reduce) for first-order labels with <= 64 path blocks per
// point: one launch fewer per label call.  DPI_FUSED_REDUCE=0 keeps the separate k_reduce launch
// (read per call, so one process can compare both).
static bool fused_reduce_on() { return env_int("DPI_FUSED_REDUCE", 1) != 0; }

// k_paths phase order policy (see the kernel, "Phase order"), read per call; DPI_ORDER overrides for
// ablations.  0: the default — all terminal-first (split instances: parked, as 5).  1: the two
// workgroups of a CU in opposite orders by workgroup slot, 2 / 3: by block index, 4: all
// terminal-last, 5: all terminal-first.  Split launches without a park (more than
// DPI_PARK_MAX_BLOCKS path blocks, OU 4 x 128 ELU) run terminal-last whatever it says.
static int path_order() { return env_int("DPI_ORDER", 0); }

// Tail units (dpi_tail_units.h, dpi_device.h paths_body): how many of a parking launch's last path
// blocks run as a T-unit and an I-unit.  Read per call.  DPI_TAIL: 0 whole blocks (the launch before
// the units), a count (capped by the park rows the call leaves free, tail_cap), unset: the default
// rule.  DPI_TAIL_ORDER: the split part as I-units then T-units (0, the default) or T-units then
// I-units (1).  DPI_TAIL_LAUNCHES=2 (tests): the second units as a launch of their own behind the
// first on the call's stream, so stream order decides which unit finishes — order 0 the T-units,
// order 1 the I-units.
// The default rule (the sweeps under profiles/tail_split_ab): three quarters of the
// device's resident workgroup slots (2 per CU: 384 of 512 on MI355X), or all the call's blocks if that
// is fewer, within the cap; a multiple of 8 where it reaches 8, so that both units of a block go to one
// XCD.  Measured on k_paths at 256 / 512 / 1,024 / 1,536 blocks (rounds_k_paths.txt, the rule against
// whole blocks): -14.3 / -0.8 / -1.5 / -1.1 %; splitting a quarter of the slots or fewer is slower than not splitting (the units then
// only lengthen the last round), and at 1,024 blocks so is splitting 640 and more.
static int tail_default(int slots, int cap) {
  const int t = std::min(cap, 3 * slots / 4);
  return t >= 8 ? t & ~7 : t;
}
static bool tail_two_launches() { return env_int("DPI_TAIL_LAUNCHES", 1) == 2; }
// Hand-off sequence numbers: one per fused launch or launch with tail units, process-wide, never 0,
// so a hand-off or join word left in a workspace by an earlier launch (or never written) does not
// match this launch's.
static std::atomic<uint32_t> g_ready_seq{0};
static uint32_t next_ready_seq() {
  uint32_t s;
  do s = g_ready_seq.fetch_add(1, std::memory_order_relaxed) + 1u;
  while (s == 0u);
  return s;
}
// Sets a.tail / a.tail_order / a.tail_seq of a k_paths or k_paths_fb launch.  Units run only where the
// kernel instance has them (Route::tail), the call has a park and asks for both estimators.
static void arm_tail(PathArgs& a, const Route& r, dpi_problem p, const WsLayout& w) {
  a.tail = 0;
  if (!r.tail || !a.park || a.flags != DPI_BOTH) return;
  const int nblk = a.n * a.nbp, nb = (p->e.nx + 3) >> 2, ng = p->e.kind == DPI_EQ_CHA ? 1 : p->e.ncomp;
  const int cap = tail_cap(nblk, (long long)w.park_rows, nb, ng);
  const char* env = std::getenv("DPI_TAIL");
  const int want = env ? std::atoi(env) : tail_default(2 * cu_count(), cap);
  a.tail = std::max(0, std::min(want, cap));
  if (!a.tail) return;
  a.tail_order = env_int("DPI_TAIL_ORDER", 0) != 0;
  a.tail_seq = next_ready_seq();
}
// A path launch with its units: one launch over [base][whole][first units][second units], or
// (tail_two_launches) the second units behind it as a launch of their own, offset in the unit map as
// k_paths_gen's ranges are in the block list.
// What dpi_launch_units reports: the calling thread's last k_paths / k_paths_fb launch.
static thread_local int g_units_tail = 0, g_units_grid = 0, g_units_launches = 0;
static int launch_units(const dpi_problem_s* p, const dpi_net_s* net, Launch q, const PathArgs& a, int nbase) {
  const int nblk = a.n * a.nbp;
  q.a = &a;
  q.nblocks = (int)tail_grid(nbase, nblk, a.tail);
  g_units_tail = a.tail;
  g_units_grid = q.nblocks;
  g_units_launches = a.tail && tail_two_launches() ? 2 : 1;
  if (!a.tail || !tail_two_launches()) return launch_unit(p, net, q);
  q.nblocks -= a.tail;
  if (int rc = launch_unit(p, net, q)) return rc;
  PathArgs a2 = a;
  a2.unit0 = tail_first(nbase, nblk, a.tail, 1);
  q.a = &a2;
  q.nblocks = a.tail;
  q.t0 = q.t1 = nullptr;
  return launch_unit(p, net, q);
}

int dpi_launch_units(int* tail, int* grid, int* launches) {
  if (!tail || !grid || !launches) return fail(DPI_ERR_ARG, "launch_units: null argument");
  *tail = g_units_tail;
  *grid = g_units_grid;
  *launches = g_units_launches;
  return 0;
}

static size_t hess_extra(int n, int M, int nx, size_t* moff = nullptr);
// Validates a label call and fills its PathArgs (the first-order calls, dpi_label_prepare and, with
// ROUTE_HESS, the Hessian-label calls: their own error texts, and the Hessian block sums and moments
// behind the layout, hess_extra).  Returns 0, or the error; *w receives the workspace layout, *r the
// call's route.
static int label_args(const LabelCall& c, WsLayout* w, PathArgs* pa, Route* r) {
  const bool hess = c.hess(), need_moments = !c.stage_only;
  const int n = c.n, M = c.M;
  int rc = route_call(c.p, c.net, c.call, r);
  if (rc) return rc;
  if (n < 0 || (n && (!c.tx || !c.ws || (need_moments && !c.moments))) || c.K < 1 || M < 1 || c.m_begin < 0 ||
      c.m_end > M || c.m_end <= c.m_begin || (c.m_begin % P) || ((c.m_end % P) && c.m_end != M) ||
      !(c.flags & DPI_BOTH) || (c.flags & ~(DPI_BOTH | DPI_PREPARED)) || c.epoch > 0xFFFFFFu)
    return fail(DPI_ERR_ARG,
                hess ? "Hessian labels: bad arguments (m range within [0, M], m_begin a multiple of 64, m_end a "
                       "multiple of 64 or M; K >= 1, flags in DPI_TERMINAL | DPI_INTEGRAL | DPI_PREPARED)"
                     : "label_moments: bad arguments (m range within [0, M], m_begin a multiple of 64, m_end a "
                       "multiple of 64 or M; K >= 1)");
  if (n == 0) return 0;
  const dpi_problem p = c.p;
  // whole 64-path blocks; the lanes of the last one at m >= m_end are dead (PathArgs::m_end)
  const int nbp = (c.m_end - c.m_begin + P - 1) / P;
  if (nbp > DPI_PATHS_PER_CALL_MAX / P)
    return fail(DPI_ERR_ARG, std::string(hess ? "Hessian labels" : "label_moments") +
                                 ": at most DPI_PATHS_PER_CALL_MAX paths per call");
  // the noise staging region only for dpi_label_prepare and the DPI_PREPARED call it feeds
  const bool noise = c.noise();
  *w = ws_layout(c.net, n, M, 1 + p->e.nx, {.noise = noise, .park = r->park});
  if (hess && c.ws_bytes < al256(w->total) + hess_extra(n, M, p->e.nx))
    return fail(DPI_ERR_WORKSPACE, noise ? "workspace too small (dpi_workspace_bytes_hessians_prepared)"
                                         : "workspace too small (dpi_workspace_bytes_hessians)");
  if (!hess && c.ws_bytes < w->total)
    return fail(DPI_ERR_WORKSPACE, c.prepared() ? "workspace too small (prepared calls: dpi_workspace_bytes_prepared)"
                                                : "workspace too small");
  char* b = c.base();
  PathArgs& a = *pa;
  std::memset(&a, 0, sizeof(a));
  a.tx = c.tx;
  a.gx = (const float*)(b + w->gx);
  a.fb = (const float*)(b + w->fb);
  a.bx = (const float*)(b + w->bx);
  a.hb = (const float*)(b + w->hb);
  a.partial = (float*)(b + w->partial);
  a.n = n;
  a.nbp = nbp;
  a.m_begin = c.m_begin;
  a.m_end = c.m_end;
  a.K = c.K;
  a.flags = c.flags & DPI_BOTH;
  a.k0 = (uint32_t)c.seed;
  a.k1 = (uint32_t)(c.seed >> 32);
  a.c3t = DPI_TAG_TERM | (c.epoch << 8);
  a.c3s = DPI_TAG_S | (c.epoch << 8);
  a.c3i = DPI_TAG_INT | (c.epoch << 8);
  a.c3q = DPI_TAG_SDGD | (c.epoch << 8);
  a.point_base = c.point_base;
  a.order = path_order();
  a.split = mlp_split(c.net) ? 1 : 0;
  // the split specialised instances' park, when it holds a row for every path block of this call
  if (r->parks && (size_t)n * nbp <= w->park_rows)
    a.park = (float*)(b + w->park);
  a.td_dt = p->td_dt;
  // the route's late refusal (dpi_label_prepare launches no unit: it leaves that to the label call)
  return need_moments && r->code ? refuse(*r) : 0;
}

// Arms the fused reduce of a path launch: k_paths' last block per point counts on the workspace's
// tickets, reduces the point's partials into the call's moments and finalizes the labels into its y.
static void arm_fused_reduce(PathArgs& a, const LabelCall& c, const WsLayout& w) {
  a.tickets = (int*)(c.base() + w.tk);
  a.rd_moments = c.moments;
  a.rd_y = c.y;
  a.rd_status = net_status(c.net);
  a.rd_invM = 1.0f / (float)c.M;
  a.rd_bound = c.bound;
  a.rd_add_g = (c.flags & DPI_TERMINAL) ? 1 : 0;
}

// The separate reduce of a path launch's block sums: the moments and, where the call has a y, the
// first-order labels in its rows.
static void launch_reduce(const LabelCall& c, const PathArgs& a) {
  const int F = 1 + c.p->e.nx;
  hipLaunchKernelGGL(k_reduce, dim3(c.n, (2 * F + 3) / 4), dim3(256), 0, c.st(), a.partial, c.n, F, a.nbp, c.moments,
                     a.gx, 1.0f / (float)c.M, (c.flags & DPI_TERMINAL) ? 1 : 0, c.bound, c.y, c.ystride(),
                     net_status(c.net));
}

static int moments_impl(const LabelCall& c) {
  WsLayout w;
  PathArgs a;
  Route r;
  int rc = label_args(c, &w, &a, &r);
  if (rc || c.n == 0) return rc;
  if (c.net->d.kind == 2) {
    if ((rc = pis_paths(c, a, w))) return rc;
  } else {
    Launch q = path_launch(r, a, c.n * a.nbp, c, w);
    if (c.noise() && stages_prepare(c.p, c.net)) a.noise = (const float*)(c.base() + w.noise);
    if (a.nbp <= 64 && fused_reduce_on()) {  // k_paths' last block per point reduces and finalizes
      if (!base_tag_ok(c.ws, c.n))
        return fail(DPI_ERR_ARG, "label_moments: no dpi_point_baseline / dpi_sample_points_baseline of these n points "
                                 "was enqueued on this workspace (the fused reduce's tickets are zeroed there)");
      arm_fused_reduce(a, c, w);
    }
    take_timer(q.t0, q.t1);  // behind the last refusal: a refused call leaves the timer armed
    arm_tail(a, r, c.p, w);
    if ((rc = launch_units(c.p, c.net, q, a, 0))) return rc;
  }
  HIPCHK(hipGetLastError());
  if (!a.tickets) launch_reduce(c, a);  // else the path launch reduced
  HIPCHK(hipGetLastError());
  return 0;
}

// The one-launch dpi_sample_with_gradients (DPI_FUSED_BASE=0: two launches; read per call).
static bool fused_base_on() { return env_int("DPI_FUSED_BASE", 1) != 0; }
// sample_with_gradients (picard/data.py:211-223) as one call.  First-order Cha / OU labels of MLP
// and zero nets (no TD; <= 64 path blocks per point, so the label reduce runs in the path launch):
// ONE k_paths launch of n base blocks (base_point: the point's draws 1-3, g(x), f_b, bx; published
// per point) ahead of the n nbp path blocks, which draw their point themselves, roll out, and wait
// for the point's record only before its first use — the baseline's latency-bound chain runs beside
// the rollouts instead of ahead of them.  Otherwise the points' draws inside the baseline launch
// (k_baseline with SampleSpec), then the rollout / label kernel.  Which pairs may take the one-launch
// form: Route::fused.  PISGradNet: dpi_sample_points_t + dpi_generate_with_gradients.
int dpi_sample_with_gradients(dpi_problem p, dpi_net net, int n, int M, int K, uint64_t seed, uint32_t epoch,
                              uint32_t point_base, float eps, int t_factors, int flags, float sample_bound, float* tx,
                              float* y, float* moments, void* ws, size_t ws_bytes, void* stream) {
  Route r;
  int rc = route_call(p, net, ROUTE_FUSED, &r);
  if (rc) return rc;
  if (n < 0 || M < 1 || K < 1 || epoch > 0xFFFFFFu || t_factors < 0 || t_factors > 4096)
    return fail(DPI_ERR_ARG, "sample_with_gradients: bad arguments (n >= 0, M, K >= 1, t_factors in [0, 4096])");
  if (n == 0) return 0;
  if (!tx || !y || !moments) return fail(DPI_ERR_ARG, "sample_with_gradients: null tx, y or moments");
  const WsLayout w = ws_layout(net, n, M, 1 + p->e.nx, {.park = r.park});
  if (!ws || ws_bytes < w.total) return fail(DPI_ERR_WORKSPACE, "workspace too small");
  if (net->d.kind == 2) {
    if ((rc = dpi_sample_points_t(p, n, seed, epoch, point_base, eps, t_factors, tx, stream))) return rc;
    return dpi_generate_with_gradients(p, net, tx, n, M, K, seed, epoch, point_base, flags, sample_bound, y, moments, ws,
                                       ws_bytes, stream);
  }
  LabelCall c{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
              .point_base = point_base, .m_begin = 0, .m_end = M, .flags = flags, .ws = ws, .ws_bytes = ws_bytes,
              .stream = stream, .moments = moments, .y = y, .bound = sample_bound};
  if (r.fused && (M + P - 1) / P <= 64 && fused_reduce_on() && fused_base_on()) {
    WsLayout wl;
    PathArgs a;
    c.call = ROUTE_FUSED;
    if ((rc = label_args(c, &wl, &a, &r))) return rc;
    arm_fused_reduce(a, c, wl);
    FusedBase fb{};
    fb.nbase = n;
    fb.rec = (float*)(c.base() + wl.rec);
    fb.ready = (unsigned long long*)(c.base() + wl.ready);
    fb.ready_seq = next_ready_seq();
    fb.smp = sample_spec(p, seed, epoch, point_base, eps, t_factors, tx);
    Launch q = path_launch(r, a, n + n * a.nbp, c, wl);
    q.fbase = &fb;
    take_timer(q.t0, q.t1);  // behind label_args' late refusal
    arm_tail(a, r, p, wl);
    if ((rc = launch_units(p, net, q, a, n))) return rc;
    HIPCHK(hipGetLastError());
    base_tag_set(ws, n);  // the base blocks zeroed the tickets and left the baseline in ws
    return 0;
  }
  if ((rc = dpi_sample_points_baseline(p, net, n, seed, epoch, point_base, eps, t_factors, tx, ws, ws_bytes, stream)))
    return rc;
  return moments_impl(c);
}

// The points (dpi_sample_points_t's draws) and their baseline (dpi_point_baseline) in ONE launch
// for MLP / zero networks: each baseline workgroup samples its own point first.
int dpi_sample_points_baseline(dpi_problem p, dpi_net net, int n, uint64_t seed, uint32_t epoch, uint32_t point_base,
                               float eps, int t_factors, float* tx, void* ws, size_t ws_bytes, void* stream) {
  Route r;
  int rc = route_call(p, net, ROUTE_BASELINE, &r);
  if (rc) return rc;
  if (n < 0 || (n && (!tx || !ws)) || epoch > 0xFFFFFFu || t_factors < 0 || t_factors > 4096)
    return fail(DPI_ERR_ARG, "sample_points_baseline: bad arguments (t_factors in [0, 4096])");
  if (n == 0) return 0;
  if (net->d.kind == 2) {
    if ((rc = dpi_sample_points_t(p, n, seed, epoch, point_base, eps, t_factors, tx, stream))) return rc;
    return dpi_point_baseline(p, net, tx, n, ws, ws_bytes, stream);
  }
  const WsLayout w = ws_layout(net, n, 0, 1 + p->e.nx, {});
  if (ws_bytes < w.partial) return fail(DPI_ERR_WORKSPACE, "workspace too small");
  Launch q = baseline_launch(r, tx, n, ws, w, (hipStream_t)stream);
  q.smp = sample_spec(p, seed, epoch, point_base, eps, t_factors, tx);
  if ((rc = launch_unit(p, net, q))) return rc;
  HIPCHK(hipGetLastError());
  base_tag_set(ws, n);
  return 0;
}

int dpi_label_prepare(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K, uint64_t seed, uint32_t epoch,
                      uint32_t point_base, int m_begin, int m_end, int flags, void* ws, size_t ws_bytes, void* stream) {
  const LabelCall c{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                    .point_base = point_base, .m_begin = m_begin, .m_end = m_end, .flags = flags & DPI_BOTH, .ws = ws,
                    .ws_bytes = ws_bytes, .stream = stream, .stage_only = true};
  WsLayout w;
  PathArgs a;
  Route r;
  int rc = label_args(c, &w, &a, &r);
  if (rc || n == 0) return rc;
  if (!stages_prepare(p, net)) return 0;  // nothing to stage: the fused path kernels do it all
  prep_tag_set(c);
  if (net->d.kind == 1) {  // GBM: phase 1's noise sums, one wave per SIMD beside the previous path launch
    int* nq = (int*)(c.base() + w.nq);
    HIPCHK(hipMemsetAsync(nq, 0, 256 + (size_t)PIS_CLAIM_SLOTS * 4, c.st()));
    a.noise = (const float*)(c.base() + w.noise);
    const int nb = (p->e.nx + 3) / 4;
    hipLaunchKernelGGL(k_noise_shared<DPI_NOISE_SHARED_UNR>, dim3(4 * cu_count() * 3), dim3(P), 0, c.st(), a, nb,
                       n * a.nbp * 8, nq, nq + 64, 1);
    HIPCHK(hipGetLastError());
    return 0;
  }
  return pis_paths(c, a, w);
}

// The prepared call's side of the DPI_PREPARED contract (PrepTag), ahead of the call's own checks.
static int check_prepared(const LabelCall& c) {
  // every label call takes the workspace's record: an unprepared one restages the workspace, so a
  // record left from an unconsumed prepare no longer describes its rows
  if (!(c.flags & DPI_PREPARED)) return prep_tag_take(c.ws), 0;
  if (c.n == 0 || !c.p || !c.net || !stages_prepare(c.p, c.net)) return 0;
  const std::optional<PrepTag> staged = prep_tag_take(c.ws);
  if (!staged) return fail(DPI_ERR_ARG, "label_moments: DPI_PREPARED without a dpi_label_prepare on this workspace");
  if (!(*staged == prep_tag(c)))
    return fail(DPI_ERR_ARG, "label_moments: DPI_PREPARED arguments differ from the dpi_label_prepare call on this "
                             "workspace (points, counters, MC range, flags, GEMM precision or workspace size)");
  return 0;
}

int dpi_label_moments(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K, uint64_t seed, uint32_t epoch,
                      uint32_t point_base, int m_begin, int m_end, int flags, float* moments, void* ws,
                      size_t ws_bytes, void* stream) {
  const LabelCall c{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                    .point_base = point_base, .m_begin = m_begin, .m_end = m_end, .flags = flags, .ws = ws,
                    .ws_bytes = ws_bytes, .stream = stream, .moments = moments};
  int rc = check_prepared(c);
  return rc ? rc : moments_impl(c);
}

int dpi_label_moments_finalize(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K, uint64_t seed,
                               uint32_t epoch, uint32_t point_base, int flags, float sample_bound, float* y,
                               float* moments, void* ws, size_t ws_bytes, void* stream) {
  if (n > 0 && !y) return fail(DPI_ERR_ARG, "label_moments_finalize: null y");
  const LabelCall c{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                    .point_base = point_base, .m_begin = 0, .m_end = M, .flags = flags, .ws = ws,
                    .ws_bytes = ws_bytes, .stream = stream, .moments = moments, .y = y, .bound = sample_bound};
  int rc = check_prepared(c);
  return rc ? rc : moments_impl(c);
}

int dpi_moments_reduce(float* parts, int n_parts, int n, int nx, float* out, void* stream) {
  if (n < 0 || (n && (!parts || !out)) || n_parts < 1 || nx < 1) return fail(DPI_ERR_ARG, "moments_reduce: bad arguments");
  if (n == 0) return 0;
  if (n_parts > 1024) return fail(DPI_ERR_ARG, "moments_reduce: at most 1024 parts");
  const int len = n * 2 * (1 + nx);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_reduce_parts, dim3((len + 3) / 4), dim3(256), 0, st, (const float*)parts, n_parts, len, out);
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_sums_reduce(const float* parts, int n_parts, size_t len, float* out, void* stream) {
  if (!parts || !out || n_parts < 1 || n_parts > 1024 || len > 0x7fffffffu)
    return fail(DPI_ERR_ARG, "sums_reduce: bad arguments (1 <= n_parts <= 1024)");
  if (len == 0) return 0;
  hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)((len + 3) / 4)), dim3(256), 0, (hipStream_t)stream, parts,
                     n_parts, (int)len, out);
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_label_finalize(dpi_problem p, const float* moments, int n, int M, int flags, float sample_bound, float* y,
                       const void* ws, size_t ws_bytes, void* stream) {
  if (!p || n < 0 || (n && (!moments || !y || !ws)) || M < 1 || ws_bytes < (size_t)n * 4)
    return fail(DPI_ERR_ARG, "label_finalize: bad arguments");
  if (n == 0) return 0;
  const int F = 1 + p->e.nx;
  hipLaunchKernelGGL(k_finalize, dim3((n * F + 255) / 256), dim3(256), 0, (hipStream_t)stream, moments,
                     (const float*)ws, n, F, 1.0f / (float)M, (flags & DPI_TERMINAL) ? 1 : 0, sample_bound, y);
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_generate_with_gradients(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K, uint64_t seed,
                                uint32_t epoch, uint32_t point_base, int flags, float sample_bound, float* y,
                                float* moments, void* ws, size_t ws_bytes, void* stream) {
  Route r;
  int rc = route_call(p, net, ROUTE_BASELINE, &r);
  if (rc) return rc;
  if (n < 0 || M < 1 || K < 1) return fail(DPI_ERR_ARG, "generate_with_gradients: bad arguments (n >= 0, M, K >= 1)");
  if (n == 0) return 0;
  const WsLayout w = ws_layout(net, n, M, 1 + p->e.nx, {.park = r.park});
  if (!ws || ws_bytes < w.total) return fail(DPI_ERR_WORKSPACE, "workspace too small");
  if (!moments) return fail(DPI_ERR_ARG, "generate_with_gradients: moments buffer (n*2*(1+nx) floats) required");
  if ((rc = dpi_point_baseline(p, net, tx, n, ws, ws_bytes, stream))) return rc;
  if (!y) return fail(DPI_ERR_ARG, "generate_with_gradients: null y");
  // moments and labels come out of the same block-reduce launch
  return moments_impl(LabelCall{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                                .point_base = point_base, .m_begin = 0, .m_end = M, .flags = flags, .ws = ws,
                                .ws_bytes = ws_bytes, .stream = stream, .moments = moments, .y = y,
                                .bound = sample_bound});
}

// ---- Malliavin Hessian labels (generate_with_gradients_and_hessians)
static int hess_tiles(int nx) {
  const int NT = (nx + 15) / 16;
  return NT * (NT + 1) / 2;
}
// [packed block sums n x nbp x TC | moments]
static size_t hess_extra(int n, int M, int nx, size_t* moff) {
  const int nbp = (M + P - 1) / P;
  const size_t sums = al256((size_t)n * nbp * hess_tiles(nx) * 256 * 4);
  if (moff) *moff = sums;
  return sums + al256((size_t)n * 2 * (1 + nx) * 4);
}

size_t dpi_workspace_bytes_hessians(dpi_problem p, dpi_net net, int n, int M) {
  if (!p || n < 0 || M < 0) return 0;
  return al256(ws_layout(net, n, M, 1 + p->e.nx, {}).total) + hess_extra(n, M, p->e.nx);
}
// the same with the GBM noise staging region (dpi_label_prepare + a DPI_PREPARED Hessian-label call)
size_t dpi_workspace_bytes_hessians_prepared(dpi_problem p, dpi_net net, int n, int M) {
  if (!p || n < 0 || M < 0) return 0;
  return al256(ws_layout(net, n, M, 1 + p->e.nx, {.noise = gbm_noise_prep(p, net)}).total) + hess_extra(n, M, p->e.nx);
}

static int hess_moments_impl(const LabelCall& c) {
  // The shared validation and PathArgs fill; a.split selects the fp16-split tangent sweeps
  // (mlp_hdiag_split) unless DPI_GEMM_F32.  label_args also sets a.order (DPI_ORDER) and a.td_dt,
  // which the Hessian-label launch ignores: k_paths reads a.order only in its non-GBM instances (the
  // split ones among them where the call has a park, a.park) and a.td_dt only under TD, and the
  // Hessian instances are GBM and non-TD.
  WsLayout w;
  PathArgs a;
  Route r;
  int rc = label_args(c, &w, &a, &r);
  if (rc || c.n == 0) return rc;
  const int n = c.n, nx = c.p->e.nx, nbp = a.nbp;
  // a prepared call (GBM): the terminal / integral noise sums were staged by dpi_label_prepare's
  // k_noise_shared in the prepared layout's noise region — the same counters and summation order as
  // the path launch's own rollout, so the labels are bitwise the unprepared call's
  if (c.noise()) a.noise = (const float*)(c.base() + w.noise);
  a.c3h1 = DPI_TAG_HTERM | (c.epoch << 8);
  a.c3h2 = DPI_TAG_HINT | (c.epoch << 8);
  a.hpart = (float*)(c.base() + al256(w.total));  // [packed block sums | moments] behind the layout (hess_extra)
  const int NT = (nx + 15) / 16;
  Launch q = path_launch(r, a, n * nbp, c, w);
  q.hess = true;
  take_timer(q.t0, q.t1);
  if ((rc = launch_unit(c.p, c.net, q))) return rc;
  HIPCHK(hipGetLastError());
  launch_reduce(c, a);
  const int bpp = hess_tiles(nx);  // 256 packed words per workgroup: one 16 x 16 tile
  hipLaunchKernelGGL(k_reduce_hess, dim3((unsigned)((n + 7) / 8) * 8 * bpp), dim3(256), 0, c.st(), a.hpart, n, nx, NT,
                     nbp, bpp, c.hessian_sums, 1.0f / (float)c.M, c.bound, c.y, c.ystride(), 1 + nx, net_status(c.net));
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_label_moments_hessians(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K, uint64_t seed,
                               uint32_t epoch, uint32_t point_base, int m_begin, int m_end, int flags, float* moments,
                               float* hessian_sums, void* ws, size_t ws_bytes, void* stream) {
  if (!hessian_sums) return fail(DPI_ERR_ARG, "label_moments_hessians: null hessian_sums");
  const LabelCall c{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                    .point_base = point_base, .m_begin = m_begin, .m_end = m_end, .flags = flags, .ws = ws,
                    .ws_bytes = ws_bytes, .stream = stream, .moments = moments, .hessian_sums = hessian_sums,
                    .call = ROUTE_HESS};
  int rc = check_prepared(c);
  return rc ? rc : hess_moments_impl(c);
}

int dpi_label_finalize_hessians(dpi_problem p, const float* moments, const float* hessian_sums, int n, int M, int flags,
                                float sample_bound, float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!p || n < 0 || (n && (!moments || !hessian_sums || !y || !ws)) || M < 1 || !(flags & DPI_BOTH) ||
      (flags & ~DPI_BOTH))
    return fail(DPI_ERR_ARG, "label_finalize_hessians: bad arguments");
  if (n == 0) return 0;
  const int nx = p->e.nx, F = 1 + nx, C = nx * nx;
  if (ws_bytes < (size_t)n * 4) return fail(DPI_ERR_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const float* gx = (const float*)ws;  // WsLayout: gx at offset 0 (written by dpi_point_baseline)
  hipLaunchKernelGGL(k_finalize_y, dim3((n * F + 255) / 256), dim3(256), 0, st, moments, gx, n, F, 1.0f / (float)M,
                     (flags & DPI_TERMINAL) ? 1 : 0, sample_bound, y, F + C);
  const size_t tot = (size_t)n * C;
  hipLaunchKernelGGL(k_finalize_hess, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, hessian_sums, n, C,
                     1.0f / (float)M, sample_bound, y, F + C, F);
  HIPCHK(hipGetLastError());
  return 0;
}

int dpi_generate_with_gradients_and_hessians(dpi_problem p, dpi_net net, const float* tx, int n, int M, int K,
                                             uint64_t seed, uint32_t epoch, uint32_t point_base, float sample_bound,
                                             float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !net) return fail(DPI_ERR_ARG, "null problem or net");
  // in this call's order: a general-family Cha / OU value net hears about the equation, after the arguments
  const Route r = pair_route(p, net, ROUTE_HESS);
  if (r.code && (r.stage == ROUTE_PAIR || (r.general && (r.head || r.term || p->e.kind == DPI_EQ_GBM)))) return refuse(r);
  int rc;
  if (n < 0 || (!y && n) || M < 1 || M > 1024 * P)
    return fail(DPI_ERR_ARG, "generate_with_gradients_and_hessians: bad arguments (1 <= M <= 65536)");
  if (n == 0) return 0;
  if (p->e.kind != DPI_EQ_GBM) return fail(DPI_ERR_UNSUPPORTED, ROUTE_HESS_EQ);
  if ((rc = dpi_point_baseline(p, net, tx, n, ws, ws_bytes, stream))) return rc;
  const WsLayout w = ws_layout(net, n, M, 1 + p->e.nx, {});
  size_t moff;
  hess_extra(n, M, p->e.nx, &moff);
  float* moments = (float*)((char*)ws + al256(w.total) + moff);
  return hess_moments_impl(LabelCall{.p = p, .net = net, .tx = tx, .n = n, .M = M, .K = K, .seed = seed, .epoch = epoch,
                                     .point_base = point_base, .m_begin = 0, .m_end = M, .flags = DPI_BOTH, .ws = ws,
                                     .ws_bytes = ws_bytes, .stream = stream, .moments = moments, .y = y,
                                     .bound = sample_bound, .call = ROUTE_HESS});
}

}  // extern "C"
