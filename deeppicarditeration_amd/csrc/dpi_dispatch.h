// Host-side handles and the (equation, network shape) -> k_paths / k_baseline instantiation
// dispatch; dpi_dispatch is instantiated once per row of the unit table (DPI_UNITS, below), each in
// a dpi_paths_*.hip unit of its own, so the families compile in parallel.
#pragma once
#include <hip/hip_ext.h>

#include "dpi_device.h"

using namespace dpi;

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

// ---- dispatch over (equation, network shape)
struct Launch {
  bool baseline = false;
  const float* tx = nullptr;
  int n = 0;
  float *gx = nullptr, *fb = nullptr, *bx = nullptr, *hb = nullptr;
  const PathArgs* a = nullptr;
  int nblocks = 0;
  hipStream_t st = nullptr;
  bool hess = false;  // k_paths in Hessian-label mode (GBM only)
  bool td = false;    // k_paths with the TD estimators (problem td_dt > 0)
  SampleSpec smp{};   // baseline: sample the points in the same launch (smp.tx != null)
  int* tickets = nullptr;  // baseline: zero the fused reduce's per-point tickets
  const FusedBase* fbase = nullptr;  // k_paths_fb: the one-launch sample_with_gradients (fused_base_ok)
  // dpi_launch_timer_arm: the path launch's own start / stop timestamps (hipExtLaunchKernel records
  // them on the dispatch packet itself — no marker packets between the launches); null: untimed
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool gen = false;         // the pair runs the general MLP family (dpi_kernels.hip pair_route)
  floatx4* stash = nullptr;  // its stash region of the workspace (path launches)
  bool head = false;        // ... in its head form (a ValueGradient / OnlyGradient net): no stash
  bool term = false;        // ... read as the terminal-enforcing ansatz
};
// The path launches (k_paths, k_paths_fb) of a Launch, with its timer events when armed.
#define DPI_PATH_LAUNCH(KERN, q, ...) \
  hipExtLaunchKernelGGL(KERN, dim3((q).nblocks), dim3(NTH), 0, (q).st, (q).t0, (q).t1, 0, __VA_ARGS__)

// TDV: the TD-estimator k_paths variants, compiled in translation units of their own
// (dpi_paths_td_*.hip): sharing a unit with the plain kernels perturbs the register allocation
// of the plain fused-MLP kernel (6 spills at 256 VGPRs instead of none at 252).
// ACT: the hidden activation (DPI_ACT_*); the Tanh k_paths family lives in units of its own too
// (dpi_paths_*_tanh.hip).  k_baseline is shape- and activation-generic (it reads net.act).
// FBV: k_paths_fb, the one-launch sample_with_gradients (q.fbase), in translation units of its own
// (dpi_paths_fb_*.hip: beside the plain kernels it perturbed their register allocation — the
// OU 4 x 128 split instance went from 255 VGPRs to 256 and 3 spilled).  Instantiated where
// fused_base_shape holds, and dpi_kernels.hip fused_base_ok selects it by the same function: Cha /
// OU with ELU, zero nets and the fp16-split MLP instances (H % 32 == 0) — except OU 4 x 128, whose
// GMM statistics beside the hand-off spill 3 VGPRs at two workgroups per CU (it keeps two launches).
constexpr bool fused_base_shape(int kind, int H, int L, bool zero, int act) {
  return kind != DPI_EQ_GBM && act == DPI_ACT_ELU && (zero || (H % 32 == 0 && !(kind == DPI_EQ_OU && H == 128 && L == 4)));
}
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
template <int KIND, int H, int L, bool Z, bool TDV, int ACT = DPI_ACT_ELU, bool FBV = false, int NXW = NXP_MAX>
void do_launch(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  if constexpr (NXW > NXP_MAX) {
    static_assert(!TDV && !FBV, "wide instances: first-order labels");
    launch_paths<KIND, H, L, Z, ACT, false, false, NXW>(p->e, net, q);
  } else if constexpr (FBV) {
    if constexpr (fused_base_shape(KIND, H, L, Z, ACT))
      DPI_PATH_LAUNCH((k_paths_fb<KIND, H, L, Z, !Z, ACT>), q, p->e, net->d, *q.a,
                         *q.fbase);
  } else if constexpr (TDV) {
    launch_paths<KIND, H, L, Z, ACT, false, true, NXW>(p->e, net, q);
  } else if (q.baseline) {
    if constexpr (ACT != DPI_ACT_ELU)
      return;  // activation-generic: the ELU units hold it (dpi_dispatch refuses it in the Tanh units first)
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
    }
  } else
    launch_paths<KIND, H, L, Z, ACT, false, false, NXW>(p->e, net, q);
}

// The (H, L) pairs with a specialised k_paths instance: H the padded width class, L the hidden layers.
// GBM keeps every weight LDS-resident: H <= 64.
#define DPI_SHAPES_GBM(X) X(64, 3) X(64, 2) X(32, 2) X(32, 3) X(16, 1) X(16, 2) X(16, 3)
#define DPI_SHAPES_FO(X) X(128, 4) X(128, 3) X(128, 2) X(64, 3) X(64, 2) X(32, 2) X(16, 1) X(16, 2) X(16, 3)
constexpr bool spec_shape(int kind, int H, int L) {
#define DPI_SHAPE(HH, LL) \
  if (H == HH && L == LL) return true;
  if (kind == DPI_EQ_GBM) {
    DPI_SHAPES_GBM(DPI_SHAPE)
  } else {
    DPI_SHAPES_FO(DPI_SHAPE)
  }
#undef DPI_SHAPE
  return false;
}

// The general MLP family's units (GENV rows of DPI_UNITS): k_paths_gen at both width caps, and — in
// the ELU units, like k_baseline — the activation-generic k_baseline_gen.
// TERMV: the terminal-enforcing twins (k_paths_term, k_baseline_term), in units of their own.
template <int KIND, int ACT, bool TERMV = false>
bool dispatch_gen(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  const NetGen& g = net->g;
  if (q.baseline) {
    if constexpr (ACT == DPI_ACT_ELU) {
      if constexpr (TERMV)
        hipLaunchKernelGGL((k_baseline_term<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                           q.bx, q.smp, q.tickets);
      else
        hipLaunchKernelGGL((k_baseline_gen<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                           q.bx, q.smp, q.tickets);
      return true;
    }
    return false;
  }
  if (q.hess || q.td || q.fbase || !q.stash) return false;
  // block ranges of at most one workgroup per stash slot, in stream order (an armed launch timer
  // brackets the first range)
  const unsigned nblocks = (unsigned)q.nblocks, slots = (unsigned)gen_slots(g.H);
  for (unsigned b0 = 0; b0 < nblocks; b0 += slots) {
    const unsigned grid = std::min(nblocks - b0, slots);
    hipEvent_t t0 = b0 ? nullptr : q.t0, t1 = b0 ? nullptr : q.t1;
    if constexpr (TERMV) {
      if (g.H == 128)
        hipExtLaunchKernelGGL((k_paths_term<KIND, 128, ACT>), dim3(grid), dim3(NTH), 0, q.st, t0, t1, 0, p->e, g, *q.a,
                              q.stash, b0);
      else
        hipExtLaunchKernelGGL((k_paths_term<KIND, 256, ACT>), dim3(grid), dim3(NTH), 0, q.st, t0, t1, 0, p->e, g, *q.a,
                              q.stash, b0);
    } else if (g.H == 128)
      hipExtLaunchKernelGGL((k_paths_gen<KIND, 128, ACT>), dim3(grid), dim3(NTH), 0, q.st, t0, t1, 0, p->e, g, *q.a,
                            q.stash, b0);
    else
      hipExtLaunchKernelGGL((k_paths_gen<KIND, 256, ACT>), dim3(grid), dim3(NTH), 0, q.st, t0, t1, 0, p->e, g, *q.a,
                            q.stash, b0);
  }
  return true;
}

// The general family's GBM units (dpi_general_gbm.h; rows gen_gbm, gen_gbm_tanh): k_paths_gbm_gen, and in
// the ELU unit the activation-generic k_baseline_gbm_gen.
template <int ACT>
bool dispatch_gen_gbm(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  const NetGen& g = net->g;
  if (g.H != 128 || g.ht > GG_H / 16) return false;  // the width-128 image, widths <= 64
  if (q.baseline) {
    if constexpr (ACT == DPI_ACT_ELU) {
      hipLaunchKernelGGL((k_baseline_gbm_gen<GG_H>), dim3(q.n), dim3(NTHB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb, q.bx, q.hb,
                         q.smp, q.tickets);
      return true;
    }
    return false;
  }
  if (q.hess || q.td || q.fbase || !q.stash || p->e.nx > NXP_MAX) return false;
  const unsigned nblocks = (unsigned)q.nblocks, slots = (unsigned)GG_SLOTS;
  for (unsigned b0 = 0; b0 < nblocks; b0 += slots) {
    const unsigned grid = std::min(nblocks - b0, slots);
    hipEvent_t t0 = b0 ? nullptr : q.t0, t1 = b0 ? nullptr : q.t1;
    hipExtLaunchKernelGGL((k_paths_gbm_gen<ACT>), dim3(grid), dim3(NTH), 0, q.st, t0, t1, 0, p->e, g, *q.a, q.stash, b0);
  }
  return true;
}

// The head units (HEADV rows of DPI_UNITS; dpi_general.h NetGenHead): HEADV = 128 / 256 holds
// k_paths_head at that width cap, one launch over all blocks; HEADV = HEAD_BASE the activation-generic
// k_baseline_head.
constexpr int HEAD_BASE = 1;
template <int KIND, int ACT, int HEADV, bool TERMV = false>
bool dispatch_head(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  const NetGenHead& g = net->hd;
  if constexpr (HEADV == HEAD_BASE) {
    if (!q.baseline) return false;
    if constexpr (TERMV)
      hipLaunchKernelGGL((k_baseline_head_term<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb,
                         q.bx, q.smp, q.tickets);
    else
      hipLaunchKernelGGL((k_baseline_head<KIND>), dim3(q.n), dim3(NTB), 0, q.st, p->e, g, q.tx, q.n, q.gx, q.fb, q.bx,
                         q.smp, q.tickets);
    return true;
  } else {
    if (q.baseline || q.hess || q.td || q.fbase || g.H != HEADV) return false;
    if constexpr (TERMV)
      DPI_PATH_LAUNCH((k_paths_head_term<KIND, HEADV, ACT>), q, p->e, g, *q.a);
    else
      DPI_PATH_LAUNCH((k_paths_head<KIND, HEADV, ACT>), q, p->e, g, *q.a);
    return true;
  }
}

template <int KIND, bool TDV = false, int ACT = DPI_ACT_ELU, bool FBV = false, int NXW = NXP_MAX, bool GENV = false,
          int HEADV = 0, bool TERMV = false>
bool dpi_dispatch(const dpi_problem_s* p, const dpi_net_s* net, const Launch& q) {
  if constexpr (GENV) {
    static_assert(!TDV && !FBV && NXW == NXP_MAX, "the general family: first-order labels, nx <= 128");
    static_assert(KIND != DPI_EQ_GBM || (HEADV == 0 && !TERMV), "GBM: value nets only");
    if constexpr (KIND == DPI_EQ_GBM)
      return dispatch_gen_gbm<ACT>(p, net, q);
    else if constexpr (HEADV != 0)
      return dispatch_head<KIND, ACT, HEADV, TERMV>(p, net, q);
    else
      return dispatch_gen<KIND, ACT, TERMV>(p, net, q);
  } else {
  static_assert(HEADV == 0 && !TERMV, "head and terminal-enforcing units are general-family units");
  if constexpr (NXW > NXP_MAX) {
    if (q.baseline || q.hess || q.fbase) return false;
  }
  if constexpr (ACT == DPI_ACT_ELU) {  // zero nets and the (activation-generic) baseline: the ELU units
    if (net->d.kind == 0) {
      do_launch<KIND, 16, 1, true, TDV, DPI_ACT_ELU, FBV, NXW>(p, net, q);
      return true;
    }
  } else {
    if (net->d.kind == 0 || q.baseline) return false;
  }
  const int H = net->d.H, L = net->d.L;
  if constexpr (!TDV && !FBV && ACT == DPI_ACT_ELU && NXW == NXP_MAX) {
    if (q.baseline) {  // the baseline kernel is shape-generic
      if (KIND == DPI_EQ_GBM && H > 64) return false;
      do_launch<KIND, 16, 1, false, false>(p, net, q);
      return true;
    }
  }
  if constexpr (KIND == DPI_EQ_GBM) {  // all weights LDS-resident: H <= 64
#define DPI_SHAPE(HH, LL)                      \
  if (H == HH && L == LL) {                    \
    do_launch<KIND, HH, LL, false, TDV, ACT, FBV, NXW>(p, net, q); \
    return true;                               \
  }
    DPI_SHAPES_GBM(DPI_SHAPE)
    return false;
  } else {
    DPI_SHAPES_FO(DPI_SHAPE)
#undef DPI_SHAPE
    return false;
  }
  }
}

// ---- the unit table: one row per dpi_paths_*.hip translation unit, keyed by dpi_dispatch's template
// arguments (KIND, TDV, ACT, FBV, NXW, GENV, HEADV, TERMV).  Each unit file holds the explicit instantiation of its row
// (DPI_UNIT_DEFINE) and nothing else; every other unit sees the row as an extern template, so a row
// without a unit fails at link time.  dpi_kernels.hip dispatch_any derives the key of a launch and
// looks it up here.
#define DPI_UNITS(X)                                                \
  X(cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)            \
  X(ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)              \
  X(gbm, DPI_EQ_GBM, false, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)            \
  X(td_cha, DPI_EQ_CHA, true, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)          \
  X(td_ou, DPI_EQ_OU, true, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)            \
  X(td_gbm, DPI_EQ_GBM, true, DPI_ACT_ELU, false, NXP_MAX, false, 0, false)          \
  X(cha_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)      \
  X(ou_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)        \
  X(gbm_tanh, DPI_EQ_GBM, false, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)      \
  X(td_cha_tanh, DPI_EQ_CHA, true, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)    \
  X(td_ou_tanh, DPI_EQ_OU, true, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)      \
  X(td_gbm_tanh, DPI_EQ_GBM, true, DPI_ACT_TANH, false, NXP_MAX, false, 0, false)    \
  X(fb_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, true, NXP_MAX, false, 0, false)          \
  X(fb_ou, DPI_EQ_OU, false, DPI_ACT_ELU, true, NXP_MAX, false, 0, false)            \
  X(wide_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXW_MAX, false, 0, false)       \
  X(wide_ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXW_MAX, false, 0, false)         \
  X(wide_gbm, DPI_EQ_GBM, false, DPI_ACT_ELU, false, NXW_MAX, false, 0, false)       \
  X(wide_cha_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXW_MAX, false, 0, false) \
  X(wide_ou_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXW_MAX, false, 0, false)   \
  X(wide_gbm_tanh, DPI_EQ_GBM, false, DPI_ACT_TANH, false, NXW_MAX, false, 0, false) \
  X(gen_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 0, false) \
  X(gen_ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 0, false) \
  X(gen_cha_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 0, false) \
  X(gen_ou_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 0, false) \
  X(gen_gbm, DPI_EQ_GBM, false, DPI_ACT_ELU, false, NXP_MAX, true, 0, false) \
  X(gen_gbm_tanh, DPI_EQ_GBM, false, DPI_ACT_TANH, false, NXP_MAX, true, 0, false) \
  X(head_cha_128, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 128, false) \
  X(head_cha_256, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 256, false) \
  X(head_ou_128, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 128, false) \
  X(head_ou_256, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 256, false) \
  X(head_cha_128_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 128, false) \
  X(head_cha_256_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 256, false) \
  X(head_ou_128_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 128, false) \
  X(head_ou_256_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 256, false) \
  X(head_base_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, HEAD_BASE, false) \
  X(head_base_ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, HEAD_BASE, false) \
  X(term_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 0, true) \
  X(term_ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 0, true) \
  X(term_cha_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 0, true) \
  X(term_ou_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 0, true) \
  X(term_head_cha_128, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 128, true) \
  X(term_head_cha_256, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, 256, true) \
  X(term_head_ou_128, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 128, true) \
  X(term_head_ou_256, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, 256, true) \
  X(term_head_cha_128_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 128, true) \
  X(term_head_cha_256_tanh, DPI_EQ_CHA, false, DPI_ACT_TANH, false, NXP_MAX, true, 256, true) \
  X(term_head_ou_128_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 128, true) \
  X(term_head_ou_256_tanh, DPI_EQ_OU, false, DPI_ACT_TANH, false, NXP_MAX, true, 256, true) \
  X(term_head_base_cha, DPI_EQ_CHA, false, DPI_ACT_ELU, false, NXP_MAX, true, HEAD_BASE, true) \
  X(term_head_base_ou, DPI_EQ_OU, false, DPI_ACT_ELU, false, NXP_MAX, true, HEAD_BASE, true)

struct Unit {
  int kind;
  bool td;
  int act;
  bool fb;
  int nxw;
  bool gen;
  int head;  // 0, or a head unit's HEADV
  bool term;  // the terminal-enforcing twin of a general-family unit
  bool (*dispatch)(const dpi_problem_s*, const dpi_net_s*, const Launch&);
  constexpr bool is(int k, bool t, int a, bool f, int w, bool g = false, int h = 0, bool tm = false) const {
    return kind == k && td == t && act == a && fb == f && nxw == w && gen == g && head == h && term == tm;
  }
};
#define DPI_UNIT_EXTERN(NAME, ...) \
  extern template bool dpi_dispatch<__VA_ARGS__>(const dpi_problem_s*, const dpi_net_s*, const Launch&);
#define DPI_UNIT_ID(NAME, ...) UNIT_##NAME,
#define DPI_UNIT_ROW(NAME, ...) {__VA_ARGS__, &dpi_dispatch<__VA_ARGS__>},
DPI_UNITS(DPI_UNIT_EXTERN)
enum UnitId { DPI_UNITS(DPI_UNIT_ID) N_UNITS };
constexpr Unit UNITS[N_UNITS] = {DPI_UNITS(DPI_UNIT_ROW)};
#undef DPI_UNIT_EXTERN
#undef DPI_UNIT_ID
#undef DPI_UNIT_ROW

constexpr bool units_distinct() {
  for (int i = 0; i < N_UNITS; ++i)
    for (int j = 0; j < i; ++j)
      if (UNITS[i].is(UNITS[j].kind, UNITS[j].td, UNITS[j].act, UNITS[j].fb, UNITS[j].nxw, UNITS[j].gen, UNITS[j].head,
                      UNITS[j].term))
        return false;
  return true;
}
static_assert(units_distinct(), "two rows of DPI_UNITS share a (KIND, TDV, ACT, FBV, NXW, GENV, HEADV, TERMV) key");

// The whole of dpi_paths_<NAME>.hip: the row's template arguments are written in DPI_UNITS only.
#define DPI_UNIT_DEFINE(NAME)                                                                                   \
  template bool dpi_dispatch<UNITS[UNIT_##NAME].kind, UNITS[UNIT_##NAME].td, UNITS[UNIT_##NAME].act,            \
                             UNITS[UNIT_##NAME].fb, UNITS[UNIT_##NAME].nxw, UNITS[UNIT_##NAME].gen,                \
                             UNITS[UNIT_##NAME].head, UNITS[UNIT_##NAME].term>(                                 \
      const dpi_problem_s*, const dpi_net_s*, const Launch&);
