// Host program of tests/test_label_call_host.py: the host side of the label calls (csrc/dpi_kernels.hip)
// with nothing behind it.  It is linked with the library's host units compiled --offload-host-only and
// defines the HIP runtime calls they make itself: device memory is host memory, a launch is counted and
// otherwise does nothing.  So every refusal, every workspace size and the workspace tags (the baseline
// record, the DPI_PREPARED record) answer as they do in the library, for Cha, OU and GBM problems alike,
// on a machine with or without a GPU.  One line per call: kind | entry point | case | rc | dpi_last_error.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../include/dpi.h"

// ---- the HIP runtime, as far as the host units call it
static int g_launches = 0;
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return (*p = std::malloc(n)) ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { return std::free(p), hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
  return (*p = std::calloc(n, 1)) ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { return std::free(p), hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { return *d = h, hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { return std::memcpy(d, s, n), hipSuccess; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int*) { return hipErrorNoDevice; }  // cu_count() keeps its default
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return ++g_launches, hipSuccess; }
hipError_t hipExtLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t, hipEvent_t, hipEvent_t, int) {
  return ++g_launches, hipSuccess;
}
}

// ---- one label call, and the entry points that take it
struct Call {
  dpi_problem p;
  dpi_net net;
  float* tx;
  int n, M, K;
  uint64_t seed;
  uint32_t epoch, point_base;
  int m_begin, m_end, flags;
  float *moments, *hessian_sums, *y;
  void* ws;
  size_t ws_bytes;
};
enum Field { RANGE = 1, FLAGS = 2, MOMENTS = 4, Y = 8, HSUM = 16 };
struct Entry {
  const char* name;
  int fields;  // the arguments it has beside the common ones
  bool hess;
  std::function<int(const Call&)> call;
};
static const float BOUND = 1e9f;
static const std::vector<Entry> ENTRIES = {
    {"label_prepare", RANGE | FLAGS, false,
     [](const Call& c) {
       return dpi_label_prepare(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, c.m_begin, c.m_end,
                                c.flags, c.ws, c.ws_bytes, nullptr);
     }},
    {"label_moments", RANGE | FLAGS | MOMENTS, false,
     [](const Call& c) {
       return dpi_label_moments(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, c.m_begin, c.m_end,
                                c.flags, c.moments, c.ws, c.ws_bytes, nullptr);
     }},
    {"label_moments_finalize", FLAGS | MOMENTS | Y, false,
     [](const Call& c) {
       return dpi_label_moments_finalize(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, c.flags, BOUND,
                                         c.y, c.moments, c.ws, c.ws_bytes, nullptr);
     }},
    {"generate_with_gradients", FLAGS | MOMENTS | Y, false,
     [](const Call& c) {
       return dpi_generate_with_gradients(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, c.flags,
                                          BOUND, c.y, c.moments, c.ws, c.ws_bytes, nullptr);
     }},
    {"sample_with_gradients", FLAGS | MOMENTS | Y, false,
     [](const Call& c) {
       return dpi_sample_with_gradients(c.p, c.net, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, 1e-3f, 0, c.flags,
                                        BOUND, c.tx, c.y, c.moments, c.ws, c.ws_bytes, nullptr);
     }},
    {"label_moments_hessians", RANGE | FLAGS | MOMENTS | HSUM, true,
     [](const Call& c) {
       return dpi_label_moments_hessians(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base, c.m_begin,
                                         c.m_end, c.flags, c.moments, c.hessian_sums, c.ws, c.ws_bytes, nullptr);
     }},
    {"generate_with_gradients_and_hessians", Y, true,
     [](const Call& c) {
       return dpi_generate_with_gradients_and_hessians(c.p, c.net, c.tx, c.n, c.M, c.K, c.seed, c.epoch, c.point_base,
                                                       BOUND, c.y, c.ws, c.ws_bytes, nullptr);
     }},
};

static void report(const char* kind, const char* entry, const std::string& what, int rc) {
  char err[512] = "";
  if (rc) dpi_last_error(err, sizeof(err));
  std::printf("%s | %s | %s | rc=%d | %s\n", kind, entry, what.c_str(), rc, err);
}

// ---- the sweep: every entry point with one bad argument at a time, on a workspace that holds no record
struct Case {
  const char* name;
  int needs;  // the entry point must have these arguments
  std::function<void(Call&)> spoil;
};
static const std::vector<Case> CASES = {
    {"good", 0, [](Call&) {}},  // first-order fused-reduce calls: a workspace with no baseline
    {"null_problem", 0, [](Call& c) { c.p = nullptr; }},
    {"null_net", 0, [](Call& c) { c.net = nullptr; }},
    {"n=-1", 0, [](Call& c) { c.n = -1; }},
    {"M=0", 0, [](Call& c) { c.M = 0; }},
    {"K=0", 0, [](Call& c) { c.K = 0; }},
    {"epoch=1<<24", 0, [](Call& c) { c.epoch = 1u << 24; }},
    {"m_begin=32", RANGE, [](Call& c) { c.m_begin = 32; }},
    {"m_end=100", RANGE, [](Call& c) { c.m_end = 100; }},  // inside a block before M
    {"m_end=192", RANGE, [](Call& c) { c.m_end = 192; }},  // > M
    {"flags=0", FLAGS, [](Call& c) { c.flags = 0; }},
    {"flags=8", FLAGS, [](Call& c) { c.flags = 8; }},
    {"null_tx", 0, [](Call& c) { c.tx = nullptr; }},
    {"null_ws", 0, [](Call& c) { c.ws = nullptr; }},
    {"null_moments", MOMENTS, [](Call& c) { c.moments = nullptr; }},
    {"null_y", Y, [](Call& c) { c.y = nullptr; }},
    {"null_hessian_sums", HSUM, [](Call& c) { c.hessian_sums = nullptr; }},
    {"prepared_stages_nothing", FLAGS, [](Call& c) { c.flags |= DPI_PREPARED; }},
    {"n=0", 0, [](Call& c) { c.n = 0; }},
    {"n=0_nulls", 0,
     [](Call& c) {
       c.n = 0, c.tx = nullptr, c.moments = c.y = nullptr, c.ws = nullptr, c.ws_bytes = 0;
     }},
    {"n=0_K=0", 0, [](Call& c) { c.n = 0, c.K = 0; }},
};

struct Buffers {
  std::vector<float> tx, moments, hsum, y;
  std::vector<char> ws;
  Call call(dpi_problem p, dpi_net net, int nx, int n, int M) {
    const size_t F = 1 + nx, C = (size_t)nx * nx;
    tx.assign(n * F, 0.f), moments.assign(n * 2 * F, 0.f), hsum.assign(n * C, 0.f), y.assign(n * (F + C), 0.f);
    ws.assign(std::max(dpi_workspace_bytes_prepared(p, net, n, M), dpi_workspace_bytes_hessians_prepared(p, net, n, M)),
              0);
    // K = 2, seed 7, epoch 1, point_base 0, the whole range [0, M), both estimators
    return Call{p, net, tx.data(), n, M, 2, 7, 1, 0, 0, M, DPI_BOTH, moments.data(), hsum.data(), y.data(), ws.data(),
                ws.size()};
  }
};

static void sizes(const char* kind, dpi_problem p, dpi_net net) {
  const int NM[4][2] = {{1, 1}, {3, 100}, {16, 4096}, {2, 65536}};
  for (const auto& nm : NM)
    std::printf("%s | sizes | n=%d M=%d | %zu %zu %zu %zu\n", kind, nm[0], nm[1],
                dpi_workspace_bytes(p, net, nm[0], nm[1]), dpi_workspace_bytes_prepared(p, net, nm[0], nm[1]),
                dpi_workspace_bytes_hessians(p, net, nm[0], nm[1]),
                dpi_workspace_bytes_hessians_prepared(p, net, nm[0], nm[1]));
}

static void sweep(const char* kind, dpi_problem p, dpi_net net, int nx) {
  Buffers buf;
  const Call good = buf.call(p, net, nx, 3, 128);
  for (const Entry& e : ENTRIES) {
    for (const Case& k : CASES) {
      if ((k.needs & e.fields) != k.needs) continue;
      Call c = good;
      k.spoil(c);
      dpi_workspace_forget(good.ws, good.ws_bytes);
      report(kind, e.name, k.name, e.call(c));
    }
    // one byte short of the size the call needs, plain and DPI_PREPARED
    for (int prepared = 0; prepared <= ((e.fields & FLAGS) ? 1 : 0); ++prepared) {
      Call c = good;
      const bool prep = prepared || !std::strcmp(e.name, "label_prepare");
      c.ws_bytes = (e.hess ? (prep ? dpi_workspace_bytes_hessians_prepared : dpi_workspace_bytes_hessians)
                           : (prep ? dpi_workspace_bytes_prepared : dpi_workspace_bytes))(p, net, c.n, c.M) - 1;
      if (prepared) c.flags |= DPI_PREPARED;
      dpi_workspace_forget(good.ws, good.ws_bytes);
      report(kind, e.name, prepared ? "ws_one_byte_short_prepared" : "ws_one_byte_short", e.call(c));
    }
  }
  sizes(kind, p, net);
}

// ---- the workspace tags, in the order tests/test_gpu_label_contract.py goes through them on the GPU
static void tags(dpi_problem cha, dpi_net zero, dpi_problem gbm, int nx) {
  const Entry& moments = ENTRIES[1];
  auto step = [](const char* what, int rc) { report("tags", "-", what, rc); };
  auto baseline = [](const Call& c) { return dpi_point_baseline(c.p, c.net, c.tx, c.n, c.ws, c.ws_bytes, nullptr); };
  {  // the baseline record: set, ok, another n, forget
    Buffers buf;
    const Call c = buf.call(cha, zero, nx, 2, 128);
    Call c3 = c;
    c3.n = 1;
    step("base: no baseline", moments.call(c));
    step("base: baseline", baseline(c));
    step("base: label call", moments.call(c));
    step("base: label call of another n", moments.call(c3));
    dpi_workspace_forget(c.ws, c.ws_bytes);
    step("base: label call after forget", moments.call(c));
  }
  // the DPI_PREPARED record, on a pair that stages (GBM, MLP [16])
  const int widths[1] = {16};
  const std::vector<float> params((size_t)(1 + nx) * 16 + 16 + 16 + 1, 0.01f);
  dpi_net mlp = nullptr, mlp2 = nullptr;
  step("create mlp", dpi_net_create_mlp(1 + nx, 1, widths, DPI_ACT_ELU, params.data(), params.size(), &mlp));
  step("create mlp 2", dpi_net_create_mlp(1 + nx, 1, widths, DPI_ACT_ELU, params.data(), params.size(), &mlp2));
  sizes("cha mlp", cha, mlp);  // with the park
  sizes("gbm mlp", gbm, mlp);  // with the noise staging region
  Buffers buf;
  const Call c = buf.call(gbm, mlp, nx, 2, 128);
  Call cp = c;
  cp.flags |= DPI_PREPARED;
  const Entry &prepare = ENTRIES[0], &hessians = ENTRIES[5];
  {  // one byte short of the sizes with the noise staging region (under TD nothing is staged, so the
     // record is not asked for and the call's own size check answers)
    Call shy = cp;
    dpi_problem_set_estimate_delta_t(gbm, 0.3);
    shy.ws_bytes = dpi_workspace_bytes_prepared(gbm, mlp, c.n, c.M) - 1;
    step("prep: TD prepared call one byte short", moments.call(shy));
    shy.ws_bytes = dpi_workspace_bytes_hessians_prepared(gbm, mlp, c.n, c.M) - 1;
    step("prep: TD prepared Hessian-label call one byte short", hessians.call(shy));
    dpi_problem_set_estimate_delta_t(gbm, 0.0);
  }
  step("prep: baseline", baseline(c));
  step("prep: prepared call without a prepare", moments.call(cp));
  const std::vector<Case> differ = {{"seed", 0, [](Call& x) { x.seed += 1; }},
                                    {"point_base", 0, [](Call& x) { x.point_base += 1; }},
                                    {"m_end", 0, [](Call& x) { x.m_end = 64; }},
                                    {"flags", 0, [](Call& x) { x.flags = DPI_TERMINAL | DPI_PREPARED; }}};
  for (const Case& k : differ) {
    Call other = cp;
    k.spoil(other);
    step("prep: prepare", prepare.call(c));
    step((std::string("prep: prepared call that differs in ") + k.name).c_str(), moments.call(other));
    step("prep: the matching call after that refusal", moments.call(cp));
  }
  step("prep: prepare", prepare.call(c));
  step("prep: the matching call", moments.call(cp));
  step("prep: the matching call again", moments.call(cp));
  step("prep: prepare", prepare.call(c));
  step("prep: an unprepared call", moments.call(c));
  step("prep: the prepared call behind it", moments.call(cp));
  // a record naming a destroyed handle is dropped: "without", not "differ"
  Call c2 = c;
  c2.net = mlp2;
  step("prep: prepare with a second net", prepare.call(c2));
  step("prep: destroy the second net", dpi_net_destroy(mlp2));
  step("prep: a prepared call after the record's net was destroyed", moments.call(cp));
  dpi_workspace_forget(c.ws, c.ws_bytes);
  step("prep: label call after forget", moments.call(c));
  dpi_net_destroy(mlp);
}

int main() {
  const int nx = 5, nc = 2;
  std::vector<double> mean(nc * nx, 0.1), var(nc * nx, 1.0), pi(nc, 0.5), w(nc * (1 + nx), 0.1), v(nc, 1.0);
  dpi_problem cha = nullptr, ou = nullptr, gbm = nullptr;
  dpi_net zero = nullptr;
  if (dpi_problem_create_cha(nx, 1.0, 5.0, 1.0, &cha) || dpi_net_create_zero(&zero) ||
      dpi_problem_create_ou(nx, 1.0, 1.0, 1.0, 0.0, 1.0, nc, mean.data(), var.data(), pi.data(), &ou) ||
      dpi_problem_create_gbm(nx, 1.0, 1.0, nc, w.data(), v.data(), &gbm)) {
    char err[512];
    dpi_last_error(err, sizeof(err));
    std::fprintf(stderr, "setup failed: %s\n", err);
    return 2;
  }
  sweep("cha", cha, zero, nx);
  sweep("ou", ou, zero, nx);
  sweep("gbm", gbm, zero, nx);
  tags(cha, zero, gbm, nx);
  std::printf("launches | %d\n", g_launches);
  dpi_net_destroy(zero);
  dpi_problem_destroy(cha), dpi_problem_destroy(ou), dpi_problem_destroy(gbm);
  return 0;
}
