// The network handles of include/dpi.h: the dpi_net_create_* entry points upload the image that
// dpi_net_image.h builds on the host and bind its descriptor to the device copy; the range guard's
// status ring; dpi_net_destroy.
#include "dpi_net_image.h"

// The net's ring of sticky status words (DPI_STATUS_*), zeroed, in host-visible memory the kernels
// write with a vector store and the host reads without a HIP call; and whether every parameter is
// finite.
static int net_init_status(dpi_net_s* n, const float* params, size_t n_params) {
  n->finite = true;
  for (size_t i = 0; i < n_params; ++i)
    if (!std::isfinite(params[i])) {
      n->finite = false;
      break;
    }
  const size_t bytes = (size_t)DPI_STATUS_SLOTS * STATUS_STRIDE * sizeof(int);
  void* h = nullptr;
  HIPCHK(hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(h, 0, bytes);
  n->status_host = (int*)h;
  void* d = nullptr;
  HIPCHK(hipHostGetDevicePointer(&d, h, 0));
  n->status = (int*)d;
  n->slot = 0;
  return 0;
}

static volatile int* status_word(dpi_net net, int slot) {
  return (volatile int*)(net->status_host + (size_t)slot * STATUS_STRIDE);
}

// A handle for a built image: the blob copied to the device, the descriptor bound to the copy.
static int net_upload(const char* who, const NetImage& img, const float* params, size_t n_params, dpi_net* out) {
  const size_t bytes = img.blob.size() * sizeof(float);
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return fail(DPI_ERR_HIP, std::string(who) + ": hipMalloc failed");
  if (hipMemcpy(d, img.blob.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return fail(DPI_ERR_HIP, std::string(who) + ": hipMemcpy failed");
  }
  auto* n = new dpi_net_s(img.net);
  n->blob = d;
  net_bind(*n, reinterpret_cast<const float*>(d));
  if (int rc = net_init_status(n, params, n_params)) {
    dpi_net_destroy(n);
    return rc;
  }
  *out = n;
  return 0;
}

static int mlp_create(int n_in, int n_hidden, const int* widths, int act, const MlpSpec& s, const float* params,
                      size_t n_params, dpi_net* out) {
  if (int rc = mlp_check(n_in, n_hidden, widths, act, s.head, params, n_params, out)) return rc;
  NetImage img;
  build_mlp(img, n_in, n_hidden, widths, act, s, params);
  return net_upload(s.head == DPI_HEAD_VALUE ? "mlp" : "mlp_head", img, params, n_params, out);
}

extern "C" {

int dpi_net_create_zero(dpi_net* out) {
  if (!out) return fail(DPI_ERR_ARG, "null out");
  auto* n = new dpi_net_s();
  std::memset(&n->d, 0, sizeof(n->d));
  n->d.kind = 0;  // u = 0 cannot overflow: no status word (creation stays host-only)
  *out = n;
  return 0;
}

int dpi_net_create_mlp(int n_in, int n_hidden, const int* widths, int act, const float* params, size_t n_params,
                       dpi_net* out) {
  return mlp_create(n_in, n_hidden, widths, act, MlpSpec{}, params, n_params, out);
}

// A gradient-head net (include/dpi.h): the general image only (dpi_general.h NetGenHead), whatever the
// widths.
int dpi_net_create_mlp_head(int n_in, int n_hidden, const int* widths, int act, int head, const float* params,
                            size_t n_params, dpi_net* out) {
  return mlp_create(n_in, n_hidden, widths, act, MlpSpec{head}, params, n_params, out);
}

// A terminal-enforcing net (include/dpi.h): the value net's or the OnlyGradient head's general image,
// marked so that the pair routes to the TERMA kernels (dpi_general.h).
int dpi_net_create_mlp_terminal(int n_in, int n_hidden, const int* widths, int act, int head, double T,
                                const float* params, size_t n_params, dpi_net* out) {
  if (head == DPI_HEAD_VALUE_GRADIENT)
    return fail(DPI_ERR_ARG, "mlp_terminal: a terminal-enforcing net is DPI_HEAD_VALUE or DPI_HEAD_GRADIENT; the "
                             "reference raises ValueError for ValueGradient (picard/solution_enforce_terminal.py:18-19)");
  if (head != DPI_HEAD_VALUE && head != DPI_HEAD_GRADIENT)
    return fail(DPI_ERR_ARG, "mlp_terminal: head must be DPI_HEAD_VALUE or DPI_HEAD_GRADIENT");
  if (!(T > 0.0) || !std::isfinite(T)) return fail(DPI_ERR_ARG, "mlp_terminal: T must be positive and finite");
  if (!out) return fail(DPI_ERR_ARG, "mlp: bad arguments");
  return mlp_create(n_in, n_hidden, widths, act, MlpSpec{head, true, T}, params, n_params, out);
}

int dpi_net_create_pisgrad(int nx, int n_hidden, const int* hidden, double T, const float* params, size_t n_params,
                           dpi_net* out) {
  if (int rc = pisgrad_check(nx, n_hidden, hidden, params, n_params, out)) return rc;
  NetImage img;
  build_pisgrad(img, nx, n_hidden, hidden, T, params);
  return net_upload("pisgrad", img, params, n_params, out);
}

int dpi_net_destroy(dpi_net net) {
  if (!net) return 0;
  prep_tags_drop(net);
  if (net->blob) (void)hipFree(net->blob);
  if (net->status_host) (void)hipHostFree(net->status_host);
  delete net;
  return 0;
}

int dpi_net_set_precision(dpi_net net, int mode) {
  if (!net || mode < -1 || mode > DPI_GEMM_AUTO) return fail(DPI_ERR_ARG, "net_set_precision: bad arguments");
  net->precision = mode;
  return 0;
}

int dpi_net_status(dpi_net net, int clear, void* stream, int* status) {
  if (!net || !status) return fail(DPI_ERR_ARG, "net_status: bad arguments");
  int v = 0;
  if (net->status_host) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    v = *status_word(net, net->slot);
    if (clear && v) *status_word(net, net->slot) = 0;
  }
  *status = v;
  return 0;
}

int dpi_net_status_slot(dpi_net net, int slot, int clear) {
  if (!net || slot < 0 || slot >= DPI_STATUS_SLOTS) return fail(DPI_ERR_ARG, "net_status_slot: bad arguments");
  net->slot = slot;
  if (clear && net->status_host) *status_word(net, slot) = 0;
  return 0;
}

int dpi_net_status_peek(dpi_net net, int slot, int* status) {
  if (!net || !status || slot < 0 || slot >= DPI_STATUS_SLOTS)
    return fail(DPI_ERR_ARG, "net_status_peek: bad arguments");
  *status = net->status_host ? *status_word(net, slot) : 0;
  return 0;
}

}  // extern "C"
