// Stand-alone host program over csrc/dpi_route.h (tests/test_route_host.py); no GPU.  Prints the route
// of every (problem, network) pair of the sweep below, one line each with the five kinds of call side by
// side, behind a legend of the refusal texts (M1, M2, ... in order of first use).  The handles are filled
// by hand, as the upload would (dpi_net_image.h build_mlp), and read through dpi_dispatch.h route_pair.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../deeppicarditeration_amd/csrc/dpi_dispatch.h"

struct Answer {
  int rc = 0, family = 0;
  std::string msg, unit = "-";
  bool general = false, head = false, term = false, stash = false, fused = false, park = false, parks = false, tail = false;
};

static Answer answer(const dpi_problem_s& p, const dpi_net_s& net, bool split, RouteCall call) {
  const Route r = route(route_pair(&p, &net, p.td_dt > 0.f, split), call);
  Answer a;
  a.rc = r.code, a.family = r.family, a.msg = std::string(r.pre) + r.msg;
  if (r.unit < N_UNITS) a.unit = UNIT_NAMES[r.unit];
  a.general = r.general, a.head = r.head, a.term = r.term, a.stash = r.stash;
  a.fused = r.fused, a.park = r.park, a.parks = r.parks, a.tail = r.tail;
  return a;
}

// ---- the sweep: one representative per branch
struct NetCase {
  std::string name;
  dpi_net_s net;
  bool split = true;
};

static dpi_net_s blank_net(int kind, int nx) {
  dpi_net_s n;
  std::memset(&n.d, 0, sizeof(n.d));
  n.d.kind = kind;
  n.d.nxp = (nx + 15) & ~15;
  n.n_in = 1 + nx;
  return n;
}

// the descriptor build_mlp gives a net of these hidden widths
static dpi_net_s mlp_net(const std::vector<int>& widths, int act, int head, bool term, float T, int nx) {
  dpi_net_s n = blank_net(1, nx);
  const int L = (int)widths.size();
  int wmax = 0;
  for (int w : widths) wmax = std::max(wmax, w);
  const int H = wmax <= 16 ? 16 : wmax <= 32 ? 32 : wmax <= 64 ? 64 : wmax <= 128 ? 128 : 256;
  const int HC = H <= 128 ? 128 : 256, nxg = (nx + 15) & ~15;
  const bool headed = head != DPI_HEAD_VALUE;
  n.spec = !headed && !term && L <= 4 && wmax <= HMAX;
  n.gen = !n.spec || !spec_shape(DPI_EQ_CHA, H, L);
  int nxp = (nx + 15) & ~15, nxp32 = (nx + 31) & ~31;
  if ((nxp32 & 127) == 96) nxp = nxp32 + 32;
  n.head = head, n.term = term, n.term_T = term ? T : 0.f;
  n.d.L = L, n.d.act = act, n.d.H = headed ? HC : H, n.d.nxp = headed ? nxg : nxp;
  if (n.gen) n.g.H = HC, n.g.L = L, n.g.nxp = nxg, n.g.act = act, n.g.ht = ((wmax + 31) & ~31) / 16;
  return n;
}

static std::string mlp_name(const std::vector<int>& widths, int act, int head, bool term) {
  std::string s = "mlp[" + std::to_string(widths[0]) + "]x" + std::to_string(widths.size());
  s += act == DPI_ACT_TANH ? ":tanh" : ":elu";
  s += head == DPI_HEAD_VALUE ? ":value" : head == DPI_HEAD_VALUE_GRADIENT ? ":valuegrad" : ":grad";
  return s + (term ? ":term" : "");
}

// Every net where a branch can turn on it: at nx = 7 and 129 (exact fp32 where the GEMM mode can matter:
// nx <= 128 without TD); at nx = 128 and 256, which only move the width checks, one net of each kind.
static std::vector<NetCase> nets_for(int nx, bool td, float T) {
  std::vector<NetCase> v;
  const bool all = nx == 7 || nx == 129, f32 = nx == 7 && !td;
  auto add = [&](std::string name, dpi_net_s n, bool split = true) { v.push_back({name + (split ? ":split" : ":f32"), n, split}); };
  add("zero", blank_net(0, nx));
  add("pisgrad", blank_net(2, nx));
  const std::vector<std::vector<int>> values = {
      {16},           {32, 32},           {32, 32, 32}, {64, 64, 64}, {128, 128}, {128, 128, 128, 128},
      std::vector<int>(8, 24), {65, 65}, {129}, std::vector<int>(8, 256)};
  for (const auto& w : values)
    for (int act : {DPI_ACT_ELU, DPI_ACT_TANH})
      for (bool split : {true, false})
        if ((split || f32) && (all || ((w.size() == 2 || w.size() == 8) && (act == DPI_ACT_ELU) == (w[0] < 128)))) add(mlp_name(w, act, DPI_HEAD_VALUE, false), mlp_net(w, act, DPI_HEAD_VALUE, false, 0.f, nx), split);
  // gradient heads and terminal-enforcing nets: both width caps, both activations
  const std::vector<int> w128 = {64, 64}, w256 = {200, 200};
  struct HeadCase {
    const std::vector<int>* w;
    int act, head;
    bool term, T_ok;
  };
  const HeadCase heads[] = {
      {&w128, DPI_ACT_ELU, DPI_HEAD_VALUE_GRADIENT, false, true}, {&w256, DPI_ACT_TANH, DPI_HEAD_VALUE_GRADIENT, false, true},
      {&w128, DPI_ACT_TANH, DPI_HEAD_GRADIENT, false, true},      {&w256, DPI_ACT_ELU, DPI_HEAD_GRADIENT, false, true},
      {&w128, DPI_ACT_ELU, DPI_HEAD_VALUE, true, true},           {&w256, DPI_ACT_TANH, DPI_HEAD_VALUE, true, true},
      {&w128, DPI_ACT_ELU, DPI_HEAD_VALUE, true, false},          {&w128, DPI_ACT_ELU, DPI_HEAD_GRADIENT, true, true},
      {&w128, DPI_ACT_TANH, DPI_HEAD_GRADIENT, true, true},       {&w256, DPI_ACT_ELU, DPI_HEAD_GRADIENT, true, true},
      {&w256, DPI_ACT_TANH, DPI_HEAD_GRADIENT, true, true},       {&w128, DPI_ACT_ELU, DPI_HEAD_GRADIENT, true, false}};
  for (const HeadCase& h : heads)
    if (all || (h.act == DPI_ACT_ELU && h.w == &w128 && h.T_ok)) add(mlp_name(*h.w, h.act, h.head, h.term) + (h.T_ok ? "" : ":otherT"),
        mlp_net(*h.w, h.act, h.head, h.term, h.T_ok ? T : 2.f * T, nx));
  // descriptors no upload gives: a wrong input width, a padded width past NXW_MAX
  dpi_net_s bad = mlp_net({32, 32}, DPI_ACT_ELU, DPI_HEAD_VALUE, false, 0.f, nx);
  bad.n_in = nx + 2;
  add("mlp[32]x2:elu:value:n_in+1", bad);
  bad.n_in = nx + 1, bad.d.nxp = NXW_MAX + 16;
  add("mlp[32]x2:elu:value:nxp272", bad);
  return v;
}

int main() {
  const char* eq_names[] = {"", "cha", "ou", "gbm"};
  const char* call_names[] = {"baseline", "paths", "hess", "fused", "family"};
  const int nxs[][2] = {{7, 0}, {7, 1}, {128, 0}, {129, 0}, {129, 1}, {256, 0}};  // (nx, TD)
  std::vector<std::string> texts, lines;
  for (int eq : {DPI_EQ_CHA, DPI_EQ_OU, DPI_EQ_GBM})
    for (auto& nt : nxs) {
      dpi_problem_s p;
      std::memset(&p.e, 0, sizeof(p.e));
      p.e.kind = eq, p.e.nx = nt[0], p.e.T = 1.0f, p.e.ncomp = 1;
      p.td_dt = nt[1] ? 0.3f : 0.f;
      for (const NetCase& nc : nets_for(nt[0], nt[1] != 0, p.e.T)) {
        char buf[512];
        std::string line;
        for (int call = ROUTE_BASELINE; call <= ROUTE_FAMILY; ++call) {
          const Answer a = answer(p, nc.net, nc.split, (RouteCall)call);
          if (call == ROUTE_BASELINE) {  // what holds for the pair (the program fails if a later call disagrees)
            std::snprintf(buf, sizeof buf, "%s nx=%d td=%d %s | general=%d head=%d term=%d fused=%d park=%d parks=%d tail=%d",
                          eq_names[eq], nt[0], nt[1], nc.name.c_str(), a.general, a.head, a.term, a.fused, a.park, a.parks,
                          a.tail);
            line = buf;
          }
          std::snprintf(buf, sizeof buf, " general=%d head=%d term=%d fused=%d park=%d parks=%d tail=%d", a.general, a.head,
                        a.term, a.fused, a.park, a.parks, a.tail);
          if (line.find(buf) == std::string::npos) return std::printf("the calls of %s disagree on the pair\n", line.c_str()), 1;
          size_t m = 0;  // 0: no refusal
          if (a.rc) {
            while (m < texts.size() && texts[m] != a.msg) ++m;
            if (m == texts.size()) texts.push_back(a.msg);
            ++m;
          }
          std::snprintf(buf, sizeof buf, " | %s rc=%d M%zu family=%d unit=%s stash=%d", call_names[call], a.rc, m, a.family,
                        a.unit.c_str(), a.stash);
          line += buf;
        }
        lines.push_back(line);
      }
    }
  for (size_t m = 0; m < texts.size(); ++m) std::printf("M%zu %s\n", m + 1, texts[m].c_str());
  for (const std::string& l : lines) std::printf("%s\n", l.c_str());
  return 0;
}
