// Which kernel serves a (problem, network) pair for one kind of call, or why none does: the unit
// table's keys (DPI_UNITS) and one pure function, route(), that every entry point of dpi_kernels.hip
// asks.  Host arithmetic only, no HIP runtime call: tests/route_host.hip sweeps it without a GPU.
// dpi_dispatch.h holds the launches behind the UnitIds.
#pragma once
#include "dpi_device.h"

using namespace dpi;

// The (H, L) pairs with a specialised k_paths instance: H the padded width class, L the hidden layers.
// GBM keeps every weight LDS-resident: H <= 64.
#define DPI_SHAPES_GBM(X) X(64, 3) X(64, 2) X(32, 2) X(32, 3) X(16, 1) X(16, 2) X(16, 3)
#define DPI_SHAPES_FO(X) X(128, 4) X(128, 3) X(128, 2) X(64, 3) X(64, 2) X(32, 2) X(16, 1) X(16, 2) X(16, 3)
#define DPI_SHAPE_IS(HH, LL) || (H == HH && L == LL)
constexpr bool spec_shape(int kind, int H, int L) {
  return kind == DPI_EQ_GBM ? false DPI_SHAPES_GBM(DPI_SHAPE_IS) : false DPI_SHAPES_FO(DPI_SHAPE_IS);
}
#undef DPI_SHAPE_IS
// The shapes k_paths_fb (the one-launch sample_with_gradients) is instantiated for: Cha / OU with ELU,
// zero nets and the fp16-split MLP instances (H % 32 == 0) — except OU 4 x 128, whose GMM statistics
// beside the hand-off spill 3 VGPRs at two workgroups per CU (it keeps two launches).
constexpr bool fused_base_shape(int kind, int H, int L, bool zero, int act) {
  return kind != DPI_EQ_GBM && act == DPI_ACT_ELU && (zero || (H % 32 == 0 && !(kind == DPI_EQ_OU && H == 128 && L == 4)));
}

// ---- the unit table: one row per dpi_paths_<NAME>.hip translation unit.  A row states what differs
// from a plain unit: first-order labels with ELU at nx <= NXP_MAX of the specialised family.
//   td:   the TD-estimator k_paths variants (beside the plain kernels they perturb the register
//         allocation of the plain fused-MLP kernel: 6 spills at 256 VGPRs instead of none at 252)
//   act:  the hidden activation; the baselines are activation-generic and live in the ELU units
//   fb:   k_paths_fb; beside the plain kernels it took OU 4 x 128 split from 255 VGPRs to 256 and 3 spilled
//   nxw:  NXW_MAX: the wide first-order instances (nx up to 256), plain k_paths only
//   gen, head, term: the general MLP family (dpi_general.h, dpi_general_gbm.h); a head unit of it, by the
//         path kernel's width cap (128 / 256) or HEAD_BASE for the baseline; the terminal-enforcing twin
constexpr int HEAD_BASE = 1;
struct UnitKey {
  int kind;
  bool td = false;
  int act = DPI_ACT_ELU;
  bool fb = false;
  int nxw = NXP_MAX;
  bool gen = false;
  int head = 0;
  bool term = false;
  constexpr UnitKey TD() const { UnitKey k = *this; k.td = true; return k; }
  constexpr UnitKey tanh() const { UnitKey k = *this; k.act = DPI_ACT_TANH; return k; }
  constexpr UnitKey FB() const { UnitKey k = *this; k.fb = true; return k; }
  constexpr UnitKey wide() const { UnitKey k = *this; k.nxw = NXW_MAX; return k; }
  constexpr UnitKey general(int h = 0) const { UnitKey k = *this; k.gen = true, k.head = h; return k; }
  constexpr UnitKey terminal(int h = 0) const { UnitKey k = general(h); k.term = true; return k; }
  constexpr bool operator==(const UnitKey& o) const {
    return kind == o.kind && td == o.td && act == o.act && fb == o.fb && nxw == o.nxw && gen == o.gen && head == o.head &&
           term == o.term;
  }
};
constexpr UnitKey U_CHA{DPI_EQ_CHA}, U_OU{DPI_EQ_OU}, U_GBM{DPI_EQ_GBM};
#define DPI_UNITS(X)                                        \
  X(cha, U_CHA)                                             \
  X(ou, U_OU)                                               \
  X(gbm, U_GBM)                                             \
  X(td_cha, U_CHA.TD())                                     \
  X(td_ou, U_OU.TD())                                       \
  X(td_gbm, U_GBM.TD())                                     \
  X(cha_tanh, U_CHA.tanh())                                 \
  X(ou_tanh, U_OU.tanh())                                   \
  X(gbm_tanh, U_GBM.tanh())                                 \
  X(td_cha_tanh, U_CHA.TD().tanh())                         \
  X(td_ou_tanh, U_OU.TD().tanh())                           \
  X(td_gbm_tanh, U_GBM.TD().tanh())                         \
  X(fb_cha, U_CHA.FB())                                     \
  X(fb_ou, U_OU.FB())                                       \
  X(wide_cha, U_CHA.wide())                                 \
  X(wide_ou, U_OU.wide())                                   \
  X(wide_gbm, U_GBM.wide())                                 \
  X(wide_cha_tanh, U_CHA.wide().tanh())                     \
  X(wide_ou_tanh, U_OU.wide().tanh())                       \
  X(wide_gbm_tanh, U_GBM.wide().tanh())                     \
  X(gen_cha, U_CHA.general())                               \
  X(gen_ou, U_OU.general())                                 \
  X(gen_cha_tanh, U_CHA.general().tanh())                   \
  X(gen_ou_tanh, U_OU.general().tanh())                     \
  X(gen_gbm, U_GBM.general())                               \
  X(gen_gbm_tanh, U_GBM.general().tanh())                   \
  X(head_cha_128, U_CHA.general(128))                       \
  X(head_cha_256, U_CHA.general(256))                       \
  X(head_ou_128, U_OU.general(128))                         \
  X(head_ou_256, U_OU.general(256))                         \
  X(head_cha_128_tanh, U_CHA.general(128).tanh())           \
  X(head_cha_256_tanh, U_CHA.general(256).tanh())           \
  X(head_ou_128_tanh, U_OU.general(128).tanh())             \
  X(head_ou_256_tanh, U_OU.general(256).tanh())             \
  X(head_base_cha, U_CHA.general(HEAD_BASE))                \
  X(head_base_ou, U_OU.general(HEAD_BASE))                  \
  X(term_cha, U_CHA.terminal())                             \
  X(term_ou, U_OU.terminal())                               \
  X(term_cha_tanh, U_CHA.terminal().tanh())                 \
  X(term_ou_tanh, U_OU.terminal().tanh())                   \
  X(term_head_cha_128, U_CHA.terminal(128))                 \
  X(term_head_cha_256, U_CHA.terminal(256))                 \
  X(term_head_ou_128, U_OU.terminal(128))                   \
  X(term_head_ou_256, U_OU.terminal(256))                   \
  X(term_head_cha_128_tanh, U_CHA.terminal(128).tanh())     \
  X(term_head_cha_256_tanh, U_CHA.terminal(256).tanh())     \
  X(term_head_ou_128_tanh, U_OU.terminal(128).tanh())       \
  X(term_head_ou_256_tanh, U_OU.terminal(256).tanh())       \
  X(term_head_base_cha, U_CHA.terminal(HEAD_BASE))          \
  X(term_head_base_ou, U_OU.terminal(HEAD_BASE))

#define DPI_UNIT_ID(NAME, KEY) UNIT_##NAME,
#define DPI_UNIT_KEY(NAME, KEY) KEY,
#define DPI_UNIT_NAME(NAME, KEY) #NAME,
enum UnitId { DPI_UNITS(DPI_UNIT_ID) N_UNITS };  // N_UNITS: no unit
constexpr UnitKey UNIT_KEYS[N_UNITS] = {DPI_UNITS(DPI_UNIT_KEY)};
constexpr const char* UNIT_NAMES[N_UNITS] = {DPI_UNITS(DPI_UNIT_NAME)};
#undef DPI_UNIT_ID
#undef DPI_UNIT_KEY
#undef DPI_UNIT_NAME

constexpr UnitId unit_of(const UnitKey& k) {
  for (int i = 0; i < N_UNITS; ++i)
    if (UNIT_KEYS[i] == k) return (UnitId)i;
  return N_UNITS;
}
constexpr bool units_distinct() {
  for (int i = 0; i < N_UNITS; ++i)
    if (unit_of(UNIT_KEYS[i]) != i) return false;
  return true;
}
static_assert(units_distinct(), "two rows of DPI_UNITS share a key");

// ---- the route
// The pair, as plain values (dpi_dispatch.h route_pair fills it from the handles).
struct RoutePair {
  int eq = 0, nx = 0;   // DPI_EQ_*, the state dimension
  bool td = false;      // ESTIMATE_DELTA_T > 0
  int net = 0;          // 0 zero, 1 MLP, 2 PISGradNet
  bool n_in_ok = true;  // the net's input width is 1 + nx
  int nxp = 0;          // its padded state dimension
  // MLP nets: the images held, the head (DPI_HEAD_*), the terminal-enforcing ansatz and whether it was built
  // for the problem's T, the specialised image's shape, the general image's, the fp16-split GEMM mode
  bool spec = false, gen = false, term = false, term_T_ok = true, split = false;
  int head = 0, H = 0, L = 0, act = 0, gH = 0, ght = 0, gL = 0, gact = 0;
};
// ROUTE_FAMILY: dpi_pair_family's question, the kernel family alone — not the limits of the image,
// of PISGradNet or of the ansatz, which the label calls report.
enum RouteCall { ROUTE_BASELINE, ROUTE_PATHS, ROUTE_HESS, ROUTE_FUSED, ROUTE_FAMILY };
// When a refusal is due: with the pair's own (every call, first), with the kind of call (before the
// call's arguments are looked at), or late, once the call's arguments and workspace have passed.
enum RouteStage { ROUTE_PAIR, ROUTE_CALL, ROUTE_LATE };
struct Route {
  int code = 0;  // 0, or the refusal: DPI_ERR_*, its text pre + msg and its stage
  const char *pre = "", *msg = "";
  RouteStage stage = ROUTE_PAIR;
  UnitId unit = N_UNITS;  // serves the call; N_UNITS on refusal, and for ROUTE_FUSED unless `fused`
  // what holds for the pair whatever the status
  int family = DPI_FAMILY_SPECIALISED;               // GENERAL: the general family serves the pair
  bool general = false, head = false, term = false;  // the launch's form: the general family, its head / terminal twins
  bool stash = false;  // the launch takes the workspace's stash
  bool fused = false;  // sample_with_gradients may take the one-launch form (k_paths_fb)
  bool park = false;   // the pair's workspace holds the park
  bool parks = false;  // ... and the pair's path launches use it (where it holds a row per block)
  bool tail = false;   // ... and may end in tail units
};

// ---- refusal texts (tests/test_route_host.py reads every string literal from here on)
// The general family's caps, applied in this order (nx <= 128 between hess and td) with the form's
// prefix; null: no such cap.
struct RouteCaps { const char *pre, *gbm, *hess, *td; };
constexpr RouteCaps CAPS_TERM = {
    "a terminal-enforcing network (PicardSolutionEnforceTerminal) runs the general MLP family, which ",
    "serves Cha and OU problems only: GBM has no terminal-enforcing instance", "has no Hessian labels",
    "has no TD estimators (ESTIMATE_DELTA_T > 0)"};
constexpr RouteCaps CAPS_HEAD = {
    "a ValueGradient / OnlyGradient network (a gradient head) runs the general MLP family, which ",
    "serves Cha and OU problems only: GBM needs the Hessian of u, which a gradient head does not give",
    "has no Hessian labels", "has no TD estimators (ESTIMATE_DELTA_T > 0)"};
constexpr RouteCaps CAPS_MLP = {
    "this network has no specialised kernel instance and the general MLP family (up to 8 hidden layers of width 256) ",
    nullptr, "has no Hessian labels",
    "has no TD estimators (ESTIMATE_DELTA_T > 0): those need at most 4 hidden layers of width 128"};
constexpr RouteCaps CAPS_GBM = {
    "this GBM network has no specialised kernel instance and the general MLP family on GBM (up to 8 hidden layers of "
    "width 64) ",
    nullptr, "has no Hessian labels (nor SUPERVISE_HESSIAN)", "has no TD estimators (ESTIMATE_DELTA_T > 0)"};
constexpr const char* ROUTE_HESS_EQ =
    "Hessian labels need a SimpleDiffusionEquationWithHessian (GBMEquationComplexExact)";

inline Route route(const RoutePair& c, RouteCall call) {
  Route r;
  const bool mlp = c.net == 1, gbm = c.eq == DPI_EQ_GBM, wide = c.nx > NXP_MAX;
  const bool baseline = call == ROUTE_BASELINE, hess = call == ROUTE_HESS, limits = call != ROUTE_FAMILY;
  // A pair with a specialised instance keeps it; any other MLP net runs the general family (it holds
  // the general image then), within that family's caps.
  const bool spec = mlp && c.spec && spec_shape(c.eq, c.H, c.L);
  r.general = mlp && c.gen && !spec;
  r.head = r.general && c.head, r.term = r.general && c.term;
  r.stash = r.general && !baseline && !r.head;
  // The one-launch form: first-order Cha / OU labels at nx <= 128 without TD, of zero nets and of the
  // fp16-split specialised instances k_paths_fb has.
  r.fused = !c.td && !wide && !r.general &&
            (c.net == 0 ? fused_base_shape(c.eq, 0, 0, true, DPI_ACT_ELU)
                        : mlp && c.split && fused_base_shape(c.eq, c.H, c.L, false, c.act));
  // The park (dpi_device.h paths_body PARK): first-order Cha / OU labels at nx <= 128 of any MLP net.
  // By problem and network kind only, not by the kernel that ends up running: the workspace size does
  // not move with the precision mode, ESTIMATE_DELTA_T or the net's widths (a caller may set the first
  // two after sizing it), and the two families' workspaces keep differing by the stash alone.  The
  // fp16-split specialised instances park, and without TD end in tail units (tail_shape: not OU 4 x 128 ELU).
  r.park = mlp && !gbm && !wide;
  r.parks = r.park && c.split && !r.general;
  r.tail = r.parks && !c.td && tail_shape(c.eq, c.H, c.L, c.act);

  auto refuse = [&r](RouteStage stage, int code, const char* pre, const char* msg) {
    r.stage = stage, r.code = code, r.pre = pre, r.msg = msg;
    return r;
  };
  if (c.net && !c.n_in_ok) return refuse(ROUTE_PAIR, DPI_ERR_ARG, "", "net input width != 1 + nx");
  if (limits && c.net && c.nxp > NXW_MAX) return refuse(ROUTE_PAIR, DPI_ERR_ARG, "", "nx too large");
  if (limits && c.net == 2 && wide)
    return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, "",
                  "PISGradNet: nx exceeds the compiled maximum state dimension 128 (NXP_MAX)");
  const RouteCaps* caps = !r.general ? nullptr : c.term ? &CAPS_TERM : c.head ? &CAPS_HEAD : gbm ? &CAPS_GBM : &CAPS_MLP;
  if (caps) {
    if (gbm && caps->gbm) return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, caps->pre, caps->gbm);
    // dpi_general_gbm.h: the width-128 image with at most 4 tiles in use
    if (caps == &CAPS_GBM && (c.gH != 128 || c.ght > GG_H / 16 || c.gL > GEN_LMAX))
      return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, CAPS_MLP.pre,
                    "serves GBM problems for hidden widths <= 64 only (up to 8 hidden layers): GBM keeps W1x and the "
                    "tangents of every layer on chip");
    if (wide) return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, caps->pre, "is compiled for nx <= 128 (NXP_MAX)");
    if (c.td) return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, caps->pre, caps->td);
  } else if (mlp && gbm && !spec) {
    // neither family: a hidden layer wider than 64 (2-4 layers up to 128 wide hold the specialised image only)
    return refuse(ROUTE_PAIR, DPI_ERR_UNSUPPORTED, "",
                  "GBM networks need every hidden layer <= 64 wide (up to 8 hidden layers): GBM keeps W1x and the "
                  "tangents of every layer on chip");
  }
  if (limits && c.term && !c.term_T_ok)
    return refuse(ROUTE_PAIR, DPI_ERR_ARG, "", "the terminal-enforcing net was built for another T than the problem's");
  if (hess) {  // GBM with MLP or zero nets of the specialised family
    if (caps) return refuse(ROUTE_CALL, DPI_ERR_UNSUPPORTED, caps->pre, caps->hess);
    if (!gbm) return refuse(ROUTE_CALL, DPI_ERR_UNSUPPORTED, "", ROUTE_HESS_EQ);
    if (c.net == 2) return refuse(ROUTE_CALL, DPI_ERR_UNSUPPORTED, "", "Hessian labels: MLP or ZeroSolution networks only");
    if (wide) return refuse(ROUTE_LATE, DPI_ERR_UNSUPPORTED, "", "Hessian labels: compiled for nx <= 128 (NXP_MAX)");
  }
  if (call == ROUTE_PATHS && c.td && wide)
    return refuse(ROUTE_LATE, DPI_ERR_UNSUPPORTED, "",
                  "label_moments: the TD estimators (ESTIMATE_DELTA_T > 0) are compiled for nx <= 128 (NXP_MAX)");
  if (r.general) r.family = DPI_FAMILY_GENERAL;

  // The unit.  PISGradNet has its own pipeline.  The baselines are shape- and activation-generic: they
  // live in the ELU units (head nets: the base units) whatever the net's activation, the problem's
  // width or TD mode.  k_paths_fb has ELU, non-TD, narrow rows only; the wide units no TD or Hessian forms.
  if (c.net == 2 || call == ROUTE_FAMILY || (call == ROUTE_FUSED && !r.fused) || (mlp && !r.general && !spec)) return r;
  UnitKey k{c.eq};
  const bool paths = call == ROUTE_PATHS;
  if (r.general) {
    k = k.general(!r.head ? 0 : baseline ? HEAD_BASE : c.gH);
    k.term = r.term;
    if (!baseline && c.gact == DPI_ACT_TANH) k.act = DPI_ACT_TANH;
  } else {
    k.fb = call == ROUTE_FUSED, k.td = paths && c.td;
    if (paths && wide) k.nxw = NXW_MAX;
    if ((paths || hess) && mlp && c.act == DPI_ACT_TANH) k.act = DPI_ACT_TANH;
  }
  r.unit = unit_of(k);
  return r;
}
