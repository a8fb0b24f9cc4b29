// Host program of tests/test_net_image_host.py: builds a network's device image (dpi_net_image.h),
// binds its descriptor to the host blob and writes every named region and scalar, read through the
// descriptor as the kernels read them.  No GPU and no HIP call.
// usage: net_image_host OUT PARAMS (mlp N_IN ACT HEAD TERM T | pisgrad NX T) WIDTH...
//   PARAMS: the raw fp32 parameter vector.  OUT: records "name type count\n" + count 4-byte values.
#include <cstdio>
#include <string>

#include "../deeppicarditeration_amd/csrc/dpi_net_image.h"

static FILE* g_out;
static const NetImage* g_img;

static void scalar(const std::string& name, const char* type, const void* v, size_t cnt = 1) {
  std::fprintf(g_out, "%s %s %zu\n", name.c_str(), type, cnt);
  std::fwrite(v, 4, cnt, g_out);
}
static void put_int(const std::string& name, int v) { scalar(name, "i32", &v); }
// a region of cnt words; a null pointer (the net has no such region) is written as empty
static void region(const std::string& name, const void* p, size_t cnt, const char* type = "f32") {
  const float *lo = g_img->blob.data(), *hi = lo + g_img->blob.size(), *q = static_cast<const float*>(p);
  if (!p) cnt = 0;
  if (p && (q < lo || q + cnt > hi)) {
    std::fprintf(stderr, "%s: region outside the blob\n", name.c_str());
    std::exit(3);
  }
  scalar(name, type, p, cnt);
}
static std::string idx(const char* name, int l) { return std::string(name) + "[" + std::to_string(l) + "]"; }

template <class Net>  // the dense image's fields; nxpT: rows of W1xT
static void dense(const std::string& pre, const Net& n, int nxpT) {
  const size_t S = n.H;
  put_int(pre + "H", n.H), put_int(pre + "L", n.L), put_int(pre + "nxp", n.nxp), put_int(pre + "act", n.act);
  region(pre + "W1x", n.W1x, S * n.nxp), region(pre + "w1t", n.w1t, S), region(pre + "b1", n.b1, S);
  region(pre + "c1", n.c1, S), region(pre + "W1xT", n.W1xT, nxpT * S);
  for (int l = 1; l < n.L; ++l) {
    region(pre + idx("W", l), n.W[l], S * S), region(pre + idx("WT", l), n.WT[l], S * S);
    region(pre + idx("b", l), n.b[l], S);
  }
  region(pre + "wout", n.wout, S), scalar(pre + "bout", "f32", &n.bout);
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  g_out = std::fopen(argv[1], "wb");
  FILE* pf = std::fopen(argv[2], "rb");
  if (!g_out || !pf) return 2;
  std::vector<float> params;
  for (float x; std::fread(&x, 4, 1, pf) == 1;) params.push_back(x);
  const std::string kind = argv[3];
  const int a0 = kind == "mlp" ? 9 : 6;
  std::vector<int> widths;
  for (int k = a0; k < argc; ++k) widths.push_back(std::atoi(argv[k]));
  NetImage img;
  g_img = &img;
  const dpi_net_s& n = img.net;
  int rc;
  if (kind == "mlp") {
    MlpSpec s{std::atoi(argv[6]), std::atoi(argv[7]) != 0, std::atof(argv[8])};
    const int n_in = std::atoi(argv[4]), act = std::atoi(argv[5]), nx32 = (n_in - 1 + 31) & ~31;
    rc = mlp_check(n_in, (int)widths.size(), widths.data(), act, s.head, params.data(), params.size(), &img);
    if (!rc) {
      build_mlp(img, n_in, (int)widths.size(), widths.data(), act, s, params.data());
      net_bind(img.net, img.blob.data());
      put_int("kind", n.d.kind), put_int("n_in", n.n_in), put_int("spec", n.spec), put_int("gen", n.gen);
      put_int("head", n.head), put_int("term", n.term), scalar("term_T", "f32", &n.term_T);
      put_int("H", n.d.H), put_int("L", n.d.L), put_int("nxp", n.d.nxp), put_int("act", n.d.act);
      if (n.spec) {
        const NetDev& d = n.d;
        const size_t H = d.H;
        put_int("nxp32", d.nxp32);
        dense("d.", d, d.nxp);
        region("d.W1xS", d.W1xS, H * d.nxp32, "u32"), region("d.W1xTS", d.W1xTS, H * d.nxp32, "u32");
        for (int l = 1; l < d.L; ++l) {
          region(idx("d.WS", l), d.WS[l], H * H, "u32"), region(idx("d.WTS", l), d.WTS[l], H * H, "u32");
          region(idx("d.WU", l), d.WU[l], H * H, "u32");
        }
        scalar("d.wus", "f32", d.wus, 4), scalar("d.hsa", "f32", d.hsa, 4), scalar("d.hsc", "f32", d.hsc, 4);
        scalar("d.hzs", "f32", d.hzs, 4), scalar("d.hbs", "f32", d.hbs, 4);
      }
      if (n.gen) put_int("g.ht", n.g.ht), dense("g.", n.g, nx32);
      if (n.head) {
        const NetGenHead& h = n.hd;
        put_int("hd.ht", h.ht), put_int("hd.value", h.value), dense("hd.", h, nx32);
        region("hd.G", h.G, (size_t)nx32 * h.H), region("hd.bg", h.bg, nx32), scalar("hd.bgsum", "f32", &h.bgsum);
      }
    }
  } else {
    const int nx = std::atoi(argv[4]), L = (int)widths.size(), C = PIS_CH;
    rc = pisgrad_check(nx, L, widths.data(), params.data(), params.size(), &img);
    if (!rc) {
      build_pisgrad(img, nx, L, widths.data(), std::atof(argv[5]), params.data());
      net_bind(img.net, img.blob.data());
      const NetPisDev& p = n.pis;
      put_int("kind", n.d.kind), put_int("n_in", n.n_in), put_int("nx", p.nx), put_int("L", p.L), put_int("nsm", p.nsm);
      scalar("h", "i32", p.h, 4), scalar("T", "f32", &p.T), scalar("smooth0", "f32", &p.smooth0);
      region("phase", p.phase, C), region("coeff", p.coeff, C), region("te0", p.te0, 2 * C * C), region("te0b", p.te0b, C);
      region("te2", p.te2, C * C), region("te2b", p.te2b, C), region("sn0", p.sn0, 2 * C * C), region("sn0b", p.sn0b, C);
      for (int j = 0; j < p.nsm; ++j) region(idx("sn", j), p.sn[j], C * C), region(idx("snb", j), p.snb[j], C);
      region("snlast", p.snlast, C), region("snlastb", p.snlastb, 1);
      for (int l = 0, in = C + nx; l <= L; ++l) {
        const int o = l < L ? p.h[l] : nx;
        region(idx("nn", l), p.nn[l], (size_t)o * in), region(idx("nnb", l), p.nnb[l], o);
        region(idx("nnT", l), p.nnT[l], (size_t)o * (l ? in : nx)), region(idx("nnbP", l), p.nnbP[l], (o + 63) & ~63);
        in = o;
      }
    }
  }
  if (rc) std::fprintf(stderr, "%d %s\n", rc, g_err.c_str());
  std::fclose(g_out);
  return rc ? 1 : 0;
}
