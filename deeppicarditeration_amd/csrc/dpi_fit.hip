// C ABI of the fit's device path (include/dpi.h: dpi_fit_workspace_bytes, dpi_fit_gradients, dpi_fit_step for
// construct_mlp value networks; dpi_fit_core_workspace_bytes, dpi_fit_core_forward, dpi_fit_core_backward
// for PISGradNet's nn_module, its layer-wise form dpi_fit_core_layers_*, and dpi_fit_shell_* for what surrounds
// it: the time networks, the g0 part and the loss); the kernels are in dpi_fit.h, dpi_fit_layers.h and
// dpi_fit_shell.h.  Not a row of the unit table: nothing here depends on a (problem, network) route.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "dpi_fit.h"
#include "dpi_fit_layers.h"
#include "dpi_fit_shell.h"
#include "dpi_host.h"

// the device functor of a problem handle (dpi_kernels.hip, which owns the handle's struct)
extern "C" DPI_HIDDEN const dpi::EqDev* problem_eq(dpi_problem p);

namespace {

using namespace dpi;

// shape checks shared by both entry points: 0, or the code with the text set
int fit_shape(int n_in, int n_hidden, const int* widths, int B) {
  if (n_in < 2 || n_hidden < 1 || !widths || B < 0)
    return fail(DPI_ERR_ARG, "fit: bad shape (n_in = 1 + nx >= 2, n_hidden >= 1, widths, B >= 0)");
  if (n_in > FIT_NIN_MAX)
    return fail(DPI_ERR_UNSUPPORTED, "fit: nx = " + std::to_string(n_in - 1) + " > 256, the state dimensions the "
                                     "fit kernels are compiled for");
  if (n_hidden > FIT_LMAX)
    return fail(DPI_ERR_UNSUPPORTED, "fit: " + std::to_string(n_hidden) + " hidden layers > 8");
  for (int l = 0; l < n_hidden; ++l) {
    if (widths[l] < 1) return fail(DPI_ERR_ARG, "fit: hidden width < 1");
    if (widths[l] > FIT_WMAX)
      return fail(DPI_ERR_UNSUPPORTED, "fit: hidden width " + std::to_string(widths[l]) + " > 256");
  }
  if (B > (1 << 24)) return fail(DPI_ERR_UNSUPPORTED, "fit: B > 2^24 rows in one batch");
  return 0;
}

// the workspace layout: fills the offsets of `a` (n, L, tiles set) and returns the float count
size_t fit_layout(FitArgs& a) {
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int L = a.L;
  size_t o = 0;
  for (int l = 0; l <= L + 1; ++l) a.offA[l] = a.offP[l] = a.offD[l] = a.offZ[l] = a.offLB[l] = 0;
  for (int l = 1; l <= L; ++l) { a.offA[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 1; l <= L; ++l) { a.offP[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 1; l <= L + 1; ++l) { a.offD[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 1; l <= L + 1; ++l) { a.offZ[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 0; l <= L; ++l) { a.offLB[l] = o; o += (size_t)a.n[l] * R; }
  o += o & 1;  // the loss partials are doubles
  a.offPart = o;
  o += 2 * (size_t)a.tiles * (a.n[0] + 1);
  return o;
}

void fit_dims(FitArgs& a, int n_in, int n_hidden, const int* widths, int B) {
  a.L = n_hidden;
  a.n[0] = n_in;
  for (int l = 0; l < n_hidden; ++l) a.n[l + 1] = widths[l];
  a.n[n_hidden + 1] = 1;
  a.B = B;
  a.tiles = (B + FIT_ROWS - 1) / FIT_ROWS;
}

// ---- the PISGradNet core (dpi_fit_core_*)

int core_shape(int nx, int n_hidden, const int* widths, int B) {
  if (nx < 1 || n_hidden < 1 || !widths || B < 0)
    return fail(DPI_ERR_ARG, "fit_core: bad shape (nx >= 1, n_hidden >= 1, widths, B >= 0)");
  if (nx > CORE_NX_MAX)
    return fail(DPI_ERR_UNSUPPORTED, "fit_core: nx = " + std::to_string(nx) + " > 128, PISGradNet's state dimensions");
  if (n_hidden > CORE_LMAX)
    return fail(DPI_ERR_UNSUPPORTED, "fit_core: " + std::to_string(n_hidden) + " hidden layers > 4");
  for (int l = 0; l < n_hidden; ++l) {
    if (widths[l] < 1) return fail(DPI_ERR_ARG, "fit_core: hidden width < 1");
    if (widths[l] > CORE_WMAX)
      return fail(DPI_ERR_UNSUPPORTED, "fit_core: hidden width " + std::to_string(widths[l]) + " > 512");
  }
  if (B > (1 << 24)) return fail(DPI_ERR_UNSUPPORTED, "fit_core: B > 2^24 rows in one batch");
  return 0;
}

void core_dims(FitCoreArgs& a, int nx, int n_hidden, const int* widths, int B) {
  a.L = n_hidden;
  a.n[0] = CORE_NT + nx;
  for (int l = 0; l < n_hidden; ++l) a.n[l + 1] = widths[l];
  a.n[n_hidden + 1] = nx;
  a.B = B;
  a.tiles = (B + FIT_ROWS - 1) / FIT_ROWS;
}

// the workspace layout of the core: fills the offsets and returns the float count
size_t core_layout(FitCoreArgs& a) {
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int L = a.L;
  size_t o = 0;
  for (int l = 0; l <= L + 1; ++l) a.offA[l] = a.offP[l] = a.offD[l] = a.offZ[l] = a.offLB[l] = 0;
  for (int l = 0; l <= L; ++l) { a.offA[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 1; l <= L; ++l) { a.offP[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 1; l <= L; ++l) { a.offD[l] = o; o += (size_t)a.n[l] * R; }
  a.offD[L + 1] = a.offA[0] + (size_t)CORE_NT * R;  // delta_{L+1} = x, the last nx units of a_0
  for (int l = 1; l <= L + 1; ++l) { a.offZ[l] = o; o += (size_t)a.n[l] * R; }
  for (int l = 0; l <= L; ++l) { a.offLB[l] = o; o += (size_t)a.n[l] * R; }
  a.offN = o;
  o += (size_t)a.n[L + 1] * R;
  return o;
}

// what the core entries of both forms check and fill: the shape, the parameter tables and the workspace
int core_begin(FitCoreArgs& a, const char* who, int nx, int n_hidden, const int* widths, int B,
               const float* const* W, const float* const* b, void* ws, size_t ws_bytes, const char* query) {
  const std::string w(who);
  if (!W || !b) return fail(DPI_ERR_ARG, w + ": null pointer table (W, b)");
  for (int l = 0; l <= n_hidden; ++l)
    if (!W[l] || !b[l]) return fail(DPI_ERR_ARG, w + ": null entry in a pointer table at layer " + std::to_string(l));
  core_dims(a, nx, n_hidden, widths, B);
  const size_t need = core_layout(a) * sizeof(float);
  if ((uintptr_t)ws % 4) return fail(DPI_ERR_ARG, w + ": the workspace must be 4-byte aligned");
  if (!ws || ws_bytes < need)
    return fail(DPI_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(ws_bytes) + " < " +
                                   std::to_string(need) + " bytes, " + query + ")");
  for (int l = 0; l <= n_hidden; ++l) {
    a.W[l] = W[l];
    a.b[l] = b[l];
  }
  a.ws = (float*)ws;
  return 0;
}

}  // namespace

extern "C" size_t dpi_fit_core_workspace_bytes(int nx, int n_hidden, const int* widths, int B) {
  if (core_shape(nx, n_hidden, widths, B)) return 0;
  FitCoreArgs a{};
  core_dims(a, nx, n_hidden, widths, B);
  return core_layout(a) * sizeof(float);
}

namespace {

// the workspace query a "workspace too small" text names, by form
constexpr const char* TILES_QUERY = "dpi_fit_core_workspace_bytes";
constexpr const char* LAYERS_QUERY = "dpi_fit_core_layers_workspace_bytes";

// the forward entry of either form as `who`: 0 with `a` ready to launch, 1 for an empty batch, or the code with
// the text set
int core_forward_begin(FitCoreArgs& a, const std::string& who, const char* query, int nx, int n_hidden,
                       const int* widths, const float* const* W, const float* const* b, const float* tau,
                       int tau_stride, const float* x, int x_stride, int B, float* sp, float* q, void* ws,
                       size_t ws_bytes) {
  int rc = core_shape(nx, n_hidden, widths, B);
  if (rc) return rc;
  if (tau_stride < CORE_NT || x_stride < nx) return fail(DPI_ERR_ARG, who + ": row stride of tau < 64 or of x < nx");
  if (B == 0) return 1;
  if (!tau || !x || !sp) return fail(DPI_ERR_ARG, who + ": null tau, x or sp");
  rc = core_begin(a, who.c_str(), nx, n_hidden, widths, B, W, b, ws, ws_bytes, query);
  if (rc) return rc;
  a.tau = tau;
  a.x = x;
  a.taustride = tau_stride;
  a.xstride = x_stride;
  a.sp = sp;
  a.q = q;
  a.grad = q ? 1 : 0;
  return 0;
}

// the backward entry of either form, as core_forward_begin; blk: k_fit_core_wgrad's workgroups
int core_backward_begin(FitCoreArgs& a, int& blk, const std::string& who, const char* query, int nx, int n_hidden,
                        const int* widths, const float* const* W, const float* const* b, float* const* dW,
                        float* const* db, const float* e, const float* r, int B, float* dtau, void* ws,
                        size_t ws_bytes) {
  int rc = core_shape(nx, n_hidden, widths, B);
  if (rc) return rc;
  if (B == 0) return 1;
  if (!dW || !db) return fail(DPI_ERR_ARG, who + ": null pointer table (dW, db)");
  for (int l = 0; l <= n_hidden; ++l)
    if (!dW[l] || !db[l]) return fail(DPI_ERR_ARG, who + ": null entry in a gradient table at layer " + std::to_string(l));
  if (!e || !dtau) return fail(DPI_ERR_ARG, who + ": null e or dtau");
  rc = core_begin(a, who.c_str(), nx, n_hidden, widths, B, W, b, ws, ws_bytes, query);
  if (rc) return rc;
  for (int l = 0; l <= n_hidden; ++l) {
    a.dW[l] = dW[l];
    a.db[l] = db[l];
  }
  a.e = e;
  a.r = r;
  a.grad = r ? 1 : 0;
  a.dtau = dtau;
  blk = 0;
  for (int l = 1; l <= n_hidden + 1; ++l) {
    a.blk0[l - 1] = blk;
    blk += ((a.n[l] + FIT_WT - 1) / FIT_WT) * ((a.n[l - 1] + FIT_WT - 1) / FIT_WT);
  }
  a.blk0[n_hidden + 1] = blk;
  return 0;
}

// one launch of the layer-wise form: layer l of `a`, `units` output units from the epilogue's first
template <int ORI, int EPI>
int launch_layer(const FitCoreArgs& a, int l, int units, hipStream_t st) {
  hipLaunchKernelGGL((k_fit_layer<ORI, EPI>), dim3(a.tiles, (units + LAY_UT - 1) / LAY_UT), dim3(LAY_NTH), 0, st, a, l);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" size_t dpi_fit_core_layers_workspace_bytes(int nx, int n_hidden, const int* widths, int B) {
  return dpi_fit_core_workspace_bytes(nx, n_hidden, widths, B);  // the same arrays, no region of its own
}

extern "C" int dpi_fit_core_layers_forward(int nx, int n_hidden, const int* widths, const float* const* W,
                                           const float* const* b, const float* tau, int tau_stride, const float* x,
                                           int x_stride, int B, float* sp, float* q, void* ws, size_t ws_bytes,
                                           void* stream) {
  FitCoreArgs a{};
  int rc = core_forward_begin(a, "fit_core_layers_forward", LAYERS_QUERY, nx, n_hidden, widths, W, b, tau, tau_stride,
                              x, x_stride, B, sp, q, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const int L = n_hidden;
  hipLaunchKernelGGL(k_fit_layers_a0, dim3(a.tiles, (a.n[0] + LAY_UT - 1) / LAY_UT), dim3(LAY_NTH), 0, st, a);
  HIPCHK(hipGetLastError());
  for (int l = 1; l <= L; ++l)  // 1. forward
    if ((rc = launch_layer<LAY_N, LAY_ACT>(a, l, a.n[l], st))) return rc;
  if ((rc = launch_layer<LAY_N, LAY_OUT>(a, L + 1, nx, st))) return rc;
  hipLaunchKernelGGL(k_fit_layers_sp, dim3(a.tiles), dim3(FIT_ROWS), 0, st, a);
  HIPCHK(hipGetLastError());
  if (!a.grad) return 0;
  for (int l = L + 1; l >= 2; --l)  // 2. adjoint
    if ((rc = launch_layer<LAY_T, LAY_ADJ>(a, l, a.n[l - 1], st))) return rc;
  return launch_layer<LAY_T, LAY_Q>(a, 1, nx, st);
}

extern "C" int dpi_fit_core_layers_backward(int nx, int n_hidden, const int* widths, const float* const* W,
                                            const float* const* b, float* const* dW, float* const* db,
                                            const float* e, const float* r, int B, float* dtau, void* ws,
                                            size_t ws_bytes, void* stream) {
  FitCoreArgs a{};
  int blk = 0;
  int rc = core_backward_begin(a, blk, "fit_core_layers_backward", LAYERS_QUERY, nx, n_hidden, widths, W, b, dW, db,
                               e, r, B, dtau, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  const int L = n_hidden;
  hipLaunchKernelGGL(k_fit_layers_seed, dim3(a.tiles, (a.n[0] + LAY_UT - 1) / LAY_UT), dim3(LAY_NTH), 0, st, a);
  HIPCHK(hipGetLastError());
  if (a.grad)
    for (int l = 1; l <= L; ++l)  // 3. tangent
      if ((rc = launch_layer<LAY_N, LAY_TAN>(a, l, a.n[l], st))) return rc;
  for (int l = L + 1; l >= 2; --l)  // 4. reverse
    if ((rc = launch_layer<LAY_T, LAY_REV>(a, l, a.n[l - 1], st))) return rc;
  if ((rc = launch_layer<LAY_T, LAY_DTAU>(a, 1, CORE_NT, st))) return rc;
  hipLaunchKernelGGL(k_fit_core_wgrad, dim3(blk), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dpi_fit_core_forward(int nx, int n_hidden, const int* widths, const float* const* W,
                                    const float* const* b, const float* tau, int tau_stride, const float* x,
                                    int x_stride, int B, float* sp, float* q, void* ws, size_t ws_bytes,
                                    void* stream) {
  FitCoreArgs a{};
  const int rc = core_forward_begin(a, "fit_core_forward", TILES_QUERY, nx, n_hidden, widths, W, b, tau, tau_stride,
                                    x, x_stride, B, sp, q, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  hipLaunchKernelGGL(k_fit_core_fwd, dim3(a.tiles), dim3(FIT_NTH), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dpi_fit_core_backward(int nx, int n_hidden, const int* widths, const float* const* W,
                                     const float* const* b, float* const* dW, float* const* db, const float* e,
                                     const float* r, int B, float* dtau, void* ws, size_t ws_bytes, void* stream) {
  FitCoreArgs a{};
  int blk = 0;
  const int rc = core_backward_begin(a, blk, "fit_core_backward", TILES_QUERY, nx, n_hidden, widths, W, b, dW, db, e,
                                     r, B, dtau, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fit_core_bwd, dim3(a.tiles), dim3(FIT_NTH), 0, st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_fit_core_wgrad, dim3(blk), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" size_t dpi_fit_workspace_bytes(int n_in, int n_hidden, const int* widths, int B) {
  if (fit_shape(n_in, n_hidden, widths, B)) return 0;
  FitArgs a{};
  fit_dims(a, n_in, n_hidden, widths, B);
  return fit_layout(a) * sizeof(float);
}

namespace {

// what dpi_fit_gradients and dpi_fit_step check and fill, as `who`: 0 with `a` ready to launch and `blk` the
// weight-gradient workgroups (the losses workgroup not counted), 1 for an empty batch, or the code with the
// text set.  grads_optional: dW and db may be NULL as whole tables (their entries of `a` are then NULL).
int fit_begin(FitArgs& a, int& blk, const char* who, bool grads_optional, int n_in, int n_hidden, const int* widths,
              int act, const float* const* W, const float* const* b, float* const* dW, float* const* db,
              const float* tx, const float* y, int y_stride, int B, float beta, int loss_kind, float clip, float c,
              float* losses, void* ws, size_t ws_bytes) {
  const std::string w(who);
  int rc = fit_shape(n_in, n_hidden, widths, B);
  if (rc) return rc;
  if (act != DPI_ACT_ELU && act != DPI_ACT_TANH)
    return fail(DPI_ERR_UNSUPPORTED, w + ": activation " + std::to_string(act) + " (DPI_ACT_ELU or "
                                     "DPI_ACT_TANH for every hidden layer)");
  if (loss_kind != DPI_FIT_LOSS_SQUARE && loss_kind != DPI_FIT_LOSS_CLIP)
    return fail(DPI_ERR_ARG, w + ": loss kind (DPI_FIT_LOSS_SQUARE or DPI_FIT_LOSS_CLIP)");
  if (loss_kind == DPI_FIT_LOSS_CLIP && !(clip > 0.f && std::isfinite(clip)))
    return fail(DPI_ERR_ARG, w + ": clip must be positive and finite");
  if (!std::isfinite(beta) || !(c >= 0.f) || !std::isfinite(c))
    return fail(DPI_ERR_ARG, w + ": beta must be finite and the gradient weight c >= 0 and finite");
  if (y_stride < n_in) return fail(DPI_ERR_ARG, w + ": y row stride < 1 + nx");
  if (B == 0) return 1;
  const bool grads = !(grads_optional && !dW && !db);
  if (!W || !b || (grads && (!dW || !db))) return fail(DPI_ERR_ARG, w + ": null pointer table (W, b, dW, db)");
  for (int l = 0; l <= n_hidden; ++l)
    if (!W[l] || !b[l] || (grads && (!dW[l] || !db[l])))
      return fail(DPI_ERR_ARG, w + ": null entry in a pointer table at layer " + std::to_string(l));
  if (!tx || !y || !losses) return fail(DPI_ERR_ARG, w + ": null tx, y or losses");
  fit_dims(a, n_in, n_hidden, widths, B);
  const size_t need = fit_layout(a) * sizeof(float);
  if ((uintptr_t)ws % 8) return fail(DPI_ERR_ARG, w + ": the workspace must be 8-byte aligned");
  if (!ws || ws_bytes < need)
    return fail(DPI_ERR_WORKSPACE, w + ": workspace too small (" + std::to_string(ws_bytes) + " < " +
                                   std::to_string(need) + " bytes, dpi_fit_workspace_bytes)");
  for (int l = 0; l <= n_hidden; ++l) {
    a.W[l] = W[l];
    a.b[l] = b[l];
    a.dW[l] = grads ? dW[l] : nullptr;
    a.db[l] = grads ? db[l] : nullptr;
  }
  a.tx = tx;
  a.y = y;
  a.ystride = y_stride;
  a.grad = c > 1e-9f ? 1 : 0;  // build_objective's threshold for the plain value fit
  a.clipped = loss_kind == DPI_FIT_LOSS_CLIP;
  a.beta = beta;
  a.clip = clip;
  a.c = c;
  a.ws = (float*)ws;
  a.losses = losses;
  blk = 0;
  for (int l = 1; l <= n_hidden + 1; ++l) {
    a.blk0[l - 1] = blk;
    blk += ((a.n[l] + FIT_WT - 1) / FIT_WT) * ((a.n[l - 1] + FIT_WT - 1) / FIT_WT);
  }
  a.blk0[n_hidden + 1] = blk;
  return 0;
}

void launch_fit_rows(const FitArgs& a, int act, hipStream_t st) {
  if (act == DPI_ACT_TANH)
    hipLaunchKernelGGL(k_fit_rows<DPI_ACT_TANH>, dim3(a.tiles), dim3(FIT_NTH), 0, st, a);
  else
    hipLaunchKernelGGL(k_fit_rows<DPI_ACT_ELU>, dim3(a.tiles), dim3(FIT_NTH), 0, st, a);
}

}  // namespace

extern "C" int dpi_fit_gradients(int n_in, int n_hidden, const int* widths, int act, const float* const* W,
                                 const float* const* b, float* const* dW, float* const* db, const float* tx,
                                 const float* y, int y_stride, int B, float beta, int loss_kind, float clip,
                                 float c, float* losses, void* ws, size_t ws_bytes, void* stream) {
  FitArgs a{};
  int blk = 0;
  const int rc = fit_begin(a, blk, "fit_gradients", false, n_in, n_hidden, widths, act, W, b, dW, db, tx, y, y_stride,
                           B, beta, loss_kind, clip, c, losses, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  hipStream_t st = (hipStream_t)stream;
  launch_fit_rows(a, act, st);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_fit_wgrad, dim3(blk + 1), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dpi_fit_step(int n_in, int n_hidden, const int* widths, int act, float* const* W, float* const* b,
                            float* const* dW, float* const* db, float* const* mW, float* const* mb,
                            float* const* vW, float* const* vb, const float* tx, const float* y, int y_stride, int B,
                            float beta, int loss_kind, float clip, float c, double lr, double beta1, double beta2,
                            double eps, double weight_decay, int decoupled, int step, float* losses, void* ws,
                            size_t ws_bytes, void* stream) {
  if (step < 1) return fail(DPI_ERR_ARG, "fit_step: step " + std::to_string(step) + " < 1 (the 1-based step count)");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return fail(DPI_ERR_ARG, "fit_step: beta1 and beta2 must lie in [0, 1)");
  if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(DPI_ERR_ARG, "fit_step: eps must be >= 0 and finite");
  if (!(lr >= 0.0) || !std::isfinite(lr)) return fail(DPI_ERR_ARG, "fit_step: lr must be >= 0 and finite");
  if (!(weight_decay >= 0.0) || !std::isfinite(weight_decay))
    return fail(DPI_ERR_ARG, "fit_step: weight_decay must be >= 0 and finite");
  FitStepArgs s{};
  int blk = 0;
  const int rc = fit_begin(s.f, blk, "fit_step", true, n_in, n_hidden, widths, act, W, b, dW, db, tx, y, y_stride, B,
                           beta, loss_kind, clip, c, losses, ws, ws_bytes);
  if (rc) return rc < 0 ? rc : 0;
  if (!mW || !mb || !vW || !vb)
    return fail(DPI_ERR_ARG, "fit_step: null moment table (exp_avg, exp_avg_sq of W and b)");
  for (int l = 0; l <= n_hidden; ++l) {
    if (!mW[l] || !mb[l] || !vW[l] || !vb[l])
      return fail(DPI_ERR_ARG, "fit_step: null entry in a moment table at layer " + std::to_string(l));
    s.o.mW[l] = mW[l];
    s.o.mb[l] = mb[l];
    s.o.vW[l] = vW[l];
    s.o.vb[l] = vb[l];
  }
  s.o.omb1 = (float)(1.0 - beta1);
  s.o.beta2 = (float)beta2;
  s.o.omb2 = (float)(1.0 - beta2);
  s.o.eps = (float)eps;
  s.o.wd = (float)weight_decay;
  s.o.decay = (float)(1.0 - lr * weight_decay);
  s.o.decoupled = decoupled ? 1 : 0;
  s.o.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
  s.o.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)step));
  hipStream_t st = (hipStream_t)stream;
  launch_fit_rows(s.f, act, st);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_fit_wgrad_step, dim3(blk + 1), dim3(256), 0, st, s);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the PISGradNet shell (dpi_fit_shell_*)

namespace {

int shell_shape(const std::string& who, int nx, int n_smooth_hidden, int B) {
  if (nx < 1 || n_smooth_hidden < 1) return fail(DPI_ERR_ARG, who + ": bad shape (nx >= 1, n_smooth_hidden >= 1)");
  if (nx > SH_NX_MAX)
    return fail(DPI_ERR_UNSUPPORTED, who + ": nx = " + std::to_string(nx) + " > 128, PISGradNet's state dimensions");
  if (n_smooth_hidden > SH_LMAX)
    return fail(DPI_ERR_UNSUPPORTED, who + ": smooth_net depth " + std::to_string(n_smooth_hidden) + " > 4 (the 64 -> 64 "
                                     "layers, len(NETWORK.NEURONS))");
  if (B < 1) return fail(DPI_ERR_ARG, who + ": B = " + std::to_string(B) + " < 1 row (the loss is a mean over the batch)");
  if (B > (1 << 24)) return fail(DPI_ERR_UNSUPPORTED, who + ": B > 2^24 rows in one batch");
  return 0;
}

// the workspace layout of the shell: the tiles' loss sums (doubles) first, then the [unit][row] arrays over
// 64 (tiles + 1) rows; fills the offsets (L, nx, tiles set) and returns the float count
size_t shell_layout(FitShellArgs& a) {
  const size_t R = (size_t)(a.tiles + 1) * FIT_ROWS;
  size_t o = 2 * (size_t)a.tiles * (1 + a.nx);
  auto take = [&](int units) { const size_t at = o; o += (size_t)units * R; return at; };
  a.offE = take(SH_NE);
  a.offAt = take(SH_NT);
  a.offPt = take(SH_NT);
  a.offZt[0] = take(SH_NT);
  a.offZt[1] = take(SH_NT);
  for (int k = 0; k <= a.L; ++k) {
    a.offAs[k] = take(SH_NT);
    a.offPs[k] = take(SH_NT);
    a.offZs[k] = take(SH_NT);
  }
  a.offZL = take(1);
  a.offDW = take(SH_NT);
  return o;
}

void shell_dims(FitShellArgs& a, int nx, int n_smooth_hidden, int B) {
  a.L = n_smooth_hidden;
  a.nx = nx;
  a.B = B;
  a.tiles = (B + FIT_ROWS - 1) / FIT_ROWS;
  a.nt = SH_NT;
  a.ne = SH_NE;
}

int shell_workspace(const std::string& who, size_t need, const void* ws, size_t ws_bytes) {
  if ((uintptr_t)ws % 8) return fail(DPI_ERR_ARG, who + ": the workspace must be 8-byte aligned");
  if (!ws || ws_bytes < need)
    return fail(DPI_ERR_WORKSPACE, who + ": workspace too small (" + std::to_string(ws_bytes) + " < " +
                                   std::to_string(need) + " bytes, dpi_fit_shell_workspace_bytes)");
  return 0;
}

// the time networks' table in state-dict order: timestep_phase, t_encoder's (W, b) x 2, smooth_net's (W, b) x (L + 2)
int shell_table_size(int L) { return 5 + 2 * (L + 2); }

int shell_params(FitShellArgs& a, const std::string& who, const float* const* params) {
  if (!params) return fail(DPI_ERR_ARG, who + ": null pointer table (params)");
  for (int k = 0; k < shell_table_size(a.L); ++k)
    if (!params[k]) return fail(DPI_ERR_ARG, who + ": null entry " + std::to_string(k) + " in the parameter table");
  a.phase = params[0];
  for (int k = 0; k < 2; ++k) {
    a.Wt[k] = params[1 + 2 * k];
    a.bt[k] = params[2 + 2 * k];
  }
  for (int k = 0; k <= a.L + 1; ++k) {
    a.Ws[k] = params[5 + 2 * k];
    a.bs[k] = params[6 + 2 * k];
  }
  return 0;
}

}  // namespace

extern "C" size_t dpi_fit_shell_workspace_bytes(int nx, int n_smooth_hidden, int B) {
  if (shell_shape("fit_shell_workspace_bytes", nx, n_smooth_hidden, B)) return 0;
  FitShellArgs a{};
  shell_dims(a, nx, n_smooth_hidden, B);
  return shell_layout(a) * sizeof(float);
}

extern "C" int dpi_fit_shell_forward(dpi_problem p, double T, int nx, int n_smooth_hidden, const float* coeff,
                                     const float* const* params, const float* tx, int tx_stride, int B, int grad,
                                     float* tau, float* s, float* res, float* res_x, void* ws, size_t ws_bytes,
                                     void* stream) {
  const std::string who = "fit_shell_forward";
  int rc = shell_shape(who, nx, n_smooth_hidden, B);
  if (rc) return rc;
  if (!std::isfinite(T)) return fail(DPI_ERR_ARG, who + ": T must be finite");
  if (tx_stride < 1 + nx) return fail(DPI_ERR_ARG, who + ": tx row stride < 1 + nx");
  FitShellArgs a{};
  shell_dims(a, nx, n_smooth_hidden, B);
  if ((rc = shell_params(a, who, params))) return rc;
  if (!coeff || !tx || !tau || !s || !res || (grad && !res_x))
    return fail(DPI_ERR_ARG, who + ": null coeff, tx, tau, s, res or (with grad) res_x");
  if ((rc = shell_workspace(who, shell_layout(a) * sizeof(float), ws, ws_bytes))) return rc;
  const EqDev* eq = problem_eq(p);
  if (!eq) return fail(DPI_ERR_ARG, who + ": null problem");
  if (eq->kind != DPI_EQ_OU)
    return fail(DPI_ERR_UNSUPPORTED, who + ": the problem is not an OU problem (dpi_problem_create_ou): g0 and its "
                                     "gradient are the OU mixture's closed forms");
  if (eq->ncomp < 1 || eq->ncomp > NSG)
    return fail(DPI_ERR_UNSUPPORTED, who + ": " + std::to_string(eq->ncomp) + " mixture components > 8 (NSG)");
  if (eq->nx != nx)
    return fail(DPI_ERR_ARG, who + ": the problem has nx = " + std::to_string(eq->nx) + ", the call " + std::to_string(nx));
  a.eq = *eq;
  a.T = T;
  a.coeff = coeff;
  a.tx = tx;
  a.txstride = tx_stride;
  a.grad = grad ? 1 : 0;
  a.tau = tau;
  a.s = s;
  a.res = res;
  a.res_x = res_x;
  a.ws = (float*)ws;
  hipLaunchKernelGGL(k_fit_shell_fwd, dim3(a.tiles + 1), dim3(FIT_NTH), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dpi_fit_shell_loss(int nx, const float* sp, const float* q, const float* s, const float* res,
                                  const float* res_x, const float* tx, int tx_stride, const float* y, int y_stride,
                                  int B, float beta, int loss_kind, float clip, float kappa, float* losses, float* e,
                                  float* r, float* sbar, void* ws, size_t ws_bytes, void* stream) {
  const std::string who = "fit_shell_loss";
  int rc = shell_shape(who, nx, 1, B);
  if (rc) return rc;
  if (loss_kind != DPI_FIT_LOSS_SQUARE && loss_kind != DPI_FIT_LOSS_CLIP)
    return fail(DPI_ERR_ARG, who + ": loss kind (DPI_FIT_LOSS_SQUARE or DPI_FIT_LOSS_CLIP)");
  if (loss_kind == DPI_FIT_LOSS_CLIP && !(clip > 0.f && std::isfinite(clip)))
    return fail(DPI_ERR_ARG, who + ": clip must be positive and finite");
  if (!std::isfinite(beta) || !(kappa >= 0.f) || !std::isfinite(kappa))
    return fail(DPI_ERR_ARG, who + ": beta must be finite and the gradient weight kappa >= 0 and finite");
  if (tx_stride < 1 + nx || y_stride < 1 + nx) return fail(DPI_ERR_ARG, who + ": row stride of tx or y < 1 + nx");
  const bool grad = kappa > 1e-9f && q;  // build_objective's threshold for the plain value fit
  if (!sp || !s || !res || !tx || !y || !losses || !e || !sbar)
    return fail(DPI_ERR_ARG, who + ": null sp, s, res, tx, y, losses, e or sbar");
  if (grad && (!res_x || !r)) return fail(DPI_ERR_ARG, who + ": null res_x or r with q given and kappa > 1e-9");
  FitShellLossArgs a{};
  a.nx = nx;
  a.B = B;
  a.tiles = (B + FIT_ROWS - 1) / FIT_ROWS;
  if ((rc = shell_workspace(who, (size_t)a.tiles * (1 + nx) * sizeof(double), ws, ws_bytes))) return rc;
  a.sp = sp;
  a.q = q;
  a.s = s;
  a.res = res;
  a.res_x = res_x;
  a.tx = tx;
  a.y = y;
  a.txstride = tx_stride;
  a.ystride = y_stride;
  a.grad = grad ? 1 : 0;
  a.clipped = loss_kind == DPI_FIT_LOSS_CLIP;
  a.beta = beta;
  a.clip = clip;
  a.kappa = kappa;
  a.losses = losses;
  a.e = e;
  a.r = r;
  a.sbar = sbar;
  a.part = (double*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fit_shell_loss, dim3(a.tiles), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_fit_shell_loss_sum, dim3(1), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dpi_fit_shell_backward(int nx, int n_smooth_hidden, const float* const* params, float* const* grads,
                                      const float* dtau, const float* sbar, int B, void* ws, size_t ws_bytes,
                                      void* stream) {
  const std::string who = "fit_shell_backward";
  int rc = shell_shape(who, nx, n_smooth_hidden, B);
  if (rc) return rc;
  FitShellArgs a{};
  shell_dims(a, nx, n_smooth_hidden, B);
  if ((rc = shell_params(a, who, params))) return rc;
  if (!grads) return fail(DPI_ERR_ARG, who + ": null pointer table (grads)");
  for (int k = 0; k < shell_table_size(a.L); ++k)
    if (!grads[k]) return fail(DPI_ERR_ARG, who + ": null entry " + std::to_string(k) + " in the gradient table");
  if (!dtau || !sbar) return fail(DPI_ERR_ARG, who + ": null dtau or sbar");
  if ((rc = shell_workspace(who, shell_layout(a) * sizeof(float), ws, ws_bytes))) return rc;
  a.dtau = dtau;
  a.sbar = sbar;
  a.ws = (float*)ws;
  const int L = a.L;
  FitShellWgradArgs w{};
  w.B = B;
  w.tiles = a.tiles;
  int n = 0;
  auto table = [&](size_t offZ, size_t offA, float* dW, float* db, int nout, int nin, int nz, int zrow, int zero_bias,
                   bool ones) {
    w.lay[n] = ShellLayer{ones ? nullptr : a.ws + offZ, a.ws + offA, dW, db, nout, nin, nz, zrow, zero_bias};
    ++n;
  };
  table(a.offZt[0], a.offE, grads[1], grads[2], SH_NT, SH_NE, SH_NT, 0, 0, false);
  table(a.offZt[1], a.offAt, grads[3], grads[4], SH_NT, SH_NT, SH_NT, 0, 0, false);
  table(a.offZs[0], a.offE, grads[5], grads[6], SH_NT, SH_NE, SH_NT, 1, 0, false);
  for (int k = 1; k <= L; ++k)
    table(a.offZs[k], a.offAs[k - 1], grads[5 + 2 * k], grads[6 + 2 * k], SH_NT, SH_NT, SH_NT, 1, 0, false);
  table(a.offZL, a.offAs[L], grads[5 + 2 * (L + 1)], grads[6 + 2 * (L + 1)], nx, SH_NT, 1, 1, 1, false);
  table(0, a.offDW, grads[0], nullptr, 1, SH_NT, 1, 1, 0, true);
  w.nlay = n;
  int blk = 0;
  for (int l = 0; l < n; ++l) {
    w.blk0[l] = blk;
    blk += ((w.lay[l].nout + FIT_WT - 1) / FIT_WT) * ((w.lay[l].nin + FIT_WT - 1) / FIT_WT);
  }
  w.blk0[n] = blk;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_fit_shell_bwd, dim3(a.tiles + 1), dim3(FIT_NTH), 0, st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_fit_shell_wgrad, dim3(blk), dim3(256), 0, st, w);
  HIPCHK(hipGetLastError());
  return 0;
}
