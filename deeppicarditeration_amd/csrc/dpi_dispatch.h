// Host-side handles and the launches behind the route's UnitIds (dpi_route.h): dpi_dispatch is
// instantiated once per row of the unit table (DPI_UNITS), each in a dpi_paths_*.hip unit of its own,
// so the families compile in parallel.  The units launch what the route chose; inside a unit the only
// choice left is the template instance (net shape, split bit, zero net, width cap).
#pragma once
#include <hip/hip_ext.h>

#include "dpi_route.h"

struct dpi_problem_s {
  EqDev e;
  float td_dt = 0.f;  // DATA.ESTIMATE_DELTA_T (dpi_problem_set_estimate_delta_t)
  float alpha_init_sqrt;
  std::vector<void*> dev;
};

struct dpi_net_s {
  NetDev d;        // d.kind: 0 zero, 1 mlp, 2 PISGradNet
  NetPisDev pis;
  // MLP nets: which device images the upload built.  spec: d's (the specialised k_paths instances:
  // L <= 4, widths <= 128); gen: g's (the general family, dpi_general.h), built for every net that has
  // no specialised first-order Cha / OU instance.  A net may hold both — (32, 3) is specialised for
  // GBM only, and the upload does not know the equation.
  NetGen g{};
  bool spec = true, gen = false;
  // head nets (dpi_net_create_mlp_head with a gradient head): the general image only, as hd (g is its
  // NetGen part); head: DPI_HEAD_*
  NetGenHead hd{};
  int head = 0;
  // terminal-enforcing nets (dpi_net_create_mlp_terminal): the general image only, g (a value net) or hd
  // (an OnlyGradient head), read as the ansatz around g; term_T: the T it was built for
  bool term = false;
  float term_T = 0.f;
  void* blob = nullptr;
  int n_in = 0;
  int precision = -1;     // DPI_GEMM_* for this net (dpi_net_set_precision); -1: the process-wide mode
  bool finite = true;     // every uploaded parameter finite
  // Range-guard ring (dpi_net_status*): DPI_STATUS_SLOTS sticky words, one per 64-B line, in
  // fine-grained pinned host memory; `status` is its device address, `status_host` the host one.
  // The label reductions store DPI_STATUS_* bits into slot `slot`, selected at enqueue time.
  int* status = nullptr;
  int* status_host = nullptr;
  int slot = 0;
};
constexpr int STATUS_STRIDE = 16;  // ints per ring slot (64 B)

// The pair as the route reads it.  td: the call uses the TD estimators; split: the net's effective
// GEMM mode is the fp16-split one.
inline RoutePair route_pair(const dpi_problem_s* p, const dpi_net_s* net, bool td, bool split) {
  RoutePair c;
  c.eq = p->e.kind, c.nx = p->e.nx, c.td = td;
  c.net = net->d.kind, c.n_in_ok = net->n_in == 1 + p->e.nx, c.nxp = net->d.nxp;
  c.spec = net->spec, c.gen = net->gen, c.head = net->head, c.split = split;
  c.term = net->term, c.term_T_ok = net->term_T == p->e.T;
  c.H = net->d.H, c.L = net->d.L, c.act = net->d.act;
  c.gH = net->g.H, c.ght = net->g.ht, c.gL = net->g.L, c.gact = net->g.act;
  return c;
}

// ---- one launch of the route's unit
struct Launch {
  UnitId unit = N_UNITS;  // the route's (dpi_route.h)
  bool baseline = false, hess = false;  // the per-point baseline; k_paths in Hessian-label mode (GBM only)
  const float* tx = nullptr;
  int n = 0;
  float *gx = nullptr, *fb = nullptr, *bx = nullptr, *hb = nullptr;
  const PathArgs* a = nullptr;
  int nblocks = 0;
  hipStream_t st = nullptr;
  SampleSpec smp{};   // baseline: sample the points in the same launch (smp.tx != null)
  int* tickets = nullptr;  // baseline: zero the fused reduce's per-point tickets
  const FusedBase* fbase = nullptr;  // k_paths_fb: the one-launch sample_with_gradients (Route::fused)
  // dpi_launch_timer_arm: the path launch's own start / stop timestamps (hipExtLaunchKernel records
  // them on the dispatch packet itself — no marker packets between the launches); null: untimed
  hipEvent_t t0 = nullptr, t1 = nullptr;
  floatx4* stash = nullptr;  // the general family's stash region of the workspace (Route::stash)
};
// The path launches (k_paths, k_paths_fb) of a Launch, with its timer events when armed.
#define DPI_PATH_LAUNCH(KERN, q, ...) \
  hipExtLaunchKernelGGL(KERN, dim3((q).nblocks), dim3(NTH), 0, (q).st, (q).t0, (q).t1, 0, __VA_ARGS__)

// TDV / ACT / FBV / NXW: the unit's td / act / fb / nxw (dpi_route.h DPI_UNITS).
// The k_paths instance of a unit's <HESS, TD, NXW> for one net shape.  The one run-time bit is the
// fp16-split mode (q.a->split), which has an instance of its own where !Z && H % 32 == 0.
template <int KIND, int H, int L, bool Z, int ACT, bool HESS, bool TD, int NXW>
void launch_paths(const EqDev& e, const dpi_net_s* net, const Launch& q) {
  if constexpr (!Z && H % 32 == 0) {
    if (q.a->split) {
      DPI_PATH_LAUNCH((k_paths<KIND, H, L, Z, true, HESS, TD, ACT, NXW>), q, e, net->d, *q.a);
      return;
    }
  }
  DPI_PATH_LAUNCH((k_paths<KIND, H, L, Z, false, HESS, TD, ACT, NXW>), q, e, net->d, *q.a);
}
// NXW > NXP_MAX: the wide first-order instances (Cha / OU, nx up to NXW_MAX; dpi_paths_wide_*.hip):
// plain k_paths only — the baseline is shape-generic, the TD / Hessian / fused-baseline forms have none.
// false: the unit holds no instance for the call.
template <int KIND, int H, int L, bool Z, bool TDV, int ACT = DPI_ACT_ELU, bool FBV = false, int NXW = NXP_MAX>
bool do_launch(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  if constexpr (NXW > NXP_MAX) {
    static_assert(!TDV && !FBV, "wide instances: first-order labels");
    launch_paths<KIND, H, L, Z, ACT, false, false, NXW>(p->e, net, q);
  } else if constexpr (FBV) {
    if constexpr (fused_base_shape(KIND, H, L, Z, ACT))
      DPI_PATH_LAUNCH((k_paths_fb<KIND, H, L, Z, !Z, ACT>), q, p->e, net->d, *q.a,
                         *q.fbase);
    else
      return false;
  } else if constexpr (TDV) {
    launch_paths<KIND, H, L, Z, ACT, false, true, NXW>(p->e, net, q);
  } else if (q.baseline) {
    if constexpr (ACT != DPI_ACT_ELU)
      return false;  // activation-generic: the ELU units hold it
    else if constexpr (KIND == DPI_EQ_GBM) {
      if (p->e.nx > NXP_MAX)  // the wide baseline (nx <= 256)
        hipLaunchKernelGGL((k_baseline_gbm<Z, NXW_MAX>), dim3(q.n), dim3(NTHB), 0, q.st, p->e, net->d, q.tx, q.n, q.gx,
                           q.fb, q.bx, q.hb, q.smp, q.tickets);
      else
        hipLaunchKernelGGL((k_baseline_gbm<Z>), dim3(q.n), dim3(NTHB), 0, q.st, p->e, net->d, q.tx, q.n, q.gx, q.fb,
                           q.bx, q.hb, q.smp, q.tickets);
    }
    else
      hipLaunchKernelGGL((k_baseline<KIND, Z>), dim3(q.n), dim3(NTB), 0, q.st, p->e, net->d, q.tx, q.n, q.gx, q.fb,
                         q.bx, q.smp, q.tickets);
  } else if (q.hess) {
    if constexpr (KIND == DPI_EQ_GBM) {
      EqDev e2 = p->e;
      e2.sdgd_v = 0;  // the Hessian estimators evaluate f with the full Hessian (data.py:856, :1262-1272)
      launch_paths<KIND, H, L, Z, ACT, true, false, NXW>(e2, net, q);
    } else
      return false;
  } else
    launch_paths<KIND, H, L, Z, ACT, false, false, NXW>(p->e, net, q);
  return true;
}

// The general family's path launch: block ranges of at most one workgroup per stash slot, in stream
// order (an armed launch timer brackets the first range).
template <class... Args>
void launch_ranges(void (*kern)(Args...), unsigned slots, const dpi_problem_s* p, const NetGen& g, const Launch& q) {
  const unsigned nblocks = (unsigned)q.nblocks;
  for (unsigned b0 = 0; b0 < nblocks; b0 += slots)
    hipExtLaunchKernelGGL(kern, dim3(std::min(nblocks - b0, slots)), dim3(NTH), 0, q.st, b0 ? nullptr : q.t0,
                          b0 ? nullptr : q.t1, 0, p->e, g, *q.a, q.stash, b0);
}

// The general MLP family's value-net units (gen rows of DPI_UNITS): k_paths_gen at both width caps
// (GBM, dpi_general_gbm.h: k_paths_gbm_gen), and — in the ELU units, like k_baseline — the
// activation-generic baseline.  TERMV: the terminal-enforcing twins, in units of their own.
template <int KIND, int ACT, bool TERMV = false>
bool dispatch_gen(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  const NetGen& g = net->g;
  if (q.baseline) {
    if constexpr (ACT != DPI_ACT_ELU)
      return false;
    else if constexpr (KIND == DPI_EQ_GBM)
      hipLaunchKernelGGL((k_baseline_gbm_gen<GG_H>), dim3(q.n), dim3(NTHB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb, q.bx, q.hb,
                         q.smp, q.tickets);
    else if constexpr (TERMV)
      hipLaunchKernelGGL((k_baseline_term<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                         q.bx, q.smp, q.tickets);
    else
      hipLaunchKernelGGL((k_baseline_gen<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                         q.bx, q.smp, q.tickets);
  } else if constexpr (KIND == DPI_EQ_GBM)
    launch_ranges(k_paths_gbm_gen<ACT>, (unsigned)GG_SLOTS, p, g, q);
  else if constexpr (TERMV)
    launch_ranges(g.H == 128 ? k_paths_term<KIND, 128, ACT> : k_paths_term<KIND, 256, ACT>, (unsigned)gen_slots(g.H), p, g, q);
  else
    launch_ranges(g.H == 128 ? k_paths_gen<KIND, 128, ACT> : k_paths_gen<KIND, 256, ACT>, (unsigned)gen_slots(g.H), p, g, q);
  return true;
}

// The head units (head rows of DPI_UNITS; dpi_general.h NetGenHead): HEADV = 128 / 256 holds
// k_paths_head at that width cap, one launch over all blocks; HEADV = HEAD_BASE the activation-generic
// k_baseline_head.
template <int KIND, int ACT, int HEADV, bool TERMV = false>
bool dispatch_head(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  const NetGenHead& g = net->hd;
  if constexpr (HEADV == HEAD_BASE) {
    if constexpr (TERMV)
      hipLaunchKernelGGL((k_baseline_head_term<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                         q.bx, q.smp, q.tickets);
    else
      hipLaunchKernelGGL((k_baseline_head<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb, q.bx,
                         q.smp, q.tickets);
  } else if constexpr (TERMV)
    DPI_PATH_LAUNCH((k_paths_head_term<KIND, HEADV, ACT>), q, p->e, g, *q.a);
  else
    DPI_PATH_LAUNCH((k_paths_head<KIND, HEADV, ACT>), q, p->e, g, *q.a);
  return true;
}

// One unit: the launch of the call q.unit was chosen for.  false: the unit holds no instance for it,
// which the route should have known (dpi_kernels.hip launch_unit reports it).
template <int KIND, bool TDV = false, int ACT = DPI_ACT_ELU, bool FBV = false, int NXW = NXP_MAX, bool GENV = false,
          int HEADV = 0, bool TERMV = false>
bool dpi_dispatch(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  if constexpr (GENV) {
    static_assert(!TDV && !FBV && NXW == NXP_MAX, "the general family: first-order labels, nx <= 128");
    static_assert(KIND != DPI_EQ_GBM || (HEADV == 0 && !TERMV), "GBM: value nets only");
    if constexpr (HEADV != 0)
      return dispatch_head<KIND, ACT, HEADV, TERMV>(p, net, q);
    else
      return dispatch_gen<KIND, ACT, TERMV>(p, net, q);
  } else {
    static_assert(HEADV == 0 && !TERMV, "head and terminal-enforcing units are general-family units");
    if (net->d.kind == 0) {  // zero nets: the ELU units
      if constexpr (ACT == DPI_ACT_ELU) return do_launch<KIND, 16, 1, true, TDV, DPI_ACT_ELU, FBV, NXW>(p, net, q);
      return false;
    }
    if constexpr (!TDV && !FBV && ACT == DPI_ACT_ELU && NXW == NXP_MAX) {
      if (q.baseline) return do_launch<KIND, 16, 1, false, false>(p, net, q);  // the baseline kernel is shape-generic
    }
    const int H = net->d.H, L = net->d.L;
#define DPI_SHAPE(HH, LL) \
  if (H == HH && L == LL) return do_launch<KIND, HH, LL, false, TDV, ACT, FBV, NXW>(p, net, q);
    if constexpr (KIND == DPI_EQ_GBM) {  // all weights LDS-resident: H <= 64
      DPI_SHAPES_GBM(DPI_SHAPE)
    } else {
      DPI_SHAPES_FO(DPI_SHAPE)
    }
#undef DPI_SHAPE
    return false;
  }
}

// ---- the units: every unit file holds the explicit instantiation of its row of DPI_UNITS
// (DPI_UNIT_DEFINE) and nothing else; every other unit sees the row as an extern template, so a row
// without a unit fails at link time.  UNIT_FNS: the launches by UnitId.
#define DPI_UNIT_ARGS(ID)                                                                                     \
  UNIT_KEYS[ID].kind, UNIT_KEYS[ID].td, UNIT_KEYS[ID].act, UNIT_KEYS[ID].fb, UNIT_KEYS[ID].nxw, UNIT_KEYS[ID].gen, \
      UNIT_KEYS[ID].head, UNIT_KEYS[ID].term
using UnitFn = bool (*)(const dpi_problem_s*, const dpi_net_s*, const Launch&);
#define DPI_UNIT_SIG(NAME) bool dpi_dispatch<DPI_UNIT_ARGS(UNIT_##NAME)>(const dpi_problem_s*, const dpi_net_s*, const Launch&)
#define DPI_UNIT_EXTERN(NAME, KEY) extern template DPI_UNIT_SIG(NAME);
#define DPI_UNIT_FN(NAME, KEY) &dpi_dispatch<DPI_UNIT_ARGS(UNIT_##NAME)>,
DPI_UNITS(DPI_UNIT_EXTERN)
constexpr UnitFn UNIT_FNS[N_UNITS] = {DPI_UNITS(DPI_UNIT_FN)};
#undef DPI_UNIT_EXTERN
#undef DPI_UNIT_FN

// The whole of dpi_paths_<NAME>.hip: the row's key is written in DPI_UNITS only.
#define DPI_UNIT_DEFINE(NAME) template DPI_UNIT_SIG(NAME);
