// The general MLP family of the first-order path kernel (Cha / OU, nx <= 128): any construct_mlp value
// network of 1..GEN_LMAX hidden layers, each 1..GEN_HMAX wide, all-ELU or all-Tanh, that has no
// specialised k_paths instance (dpi_route.h spec_shape).  Included by dpi_device.h.
//
// The specialised mlp_tile keeps every layer's activations in registers (L x H/16 x 4 per lane), which
// ends at 4 x 128.  Here the layer count is a run-time loop and registers hold two layers only — the
// one being consumed (the MFMA B operand) and the one being produced: 2 x HCAP/16 x 4 values per lane.
// What the backward pass needs of each layer, act'(a_l), is computed once in the forward pass and
// parked in a stash in global memory: every lane writes and later reads back its own fragments as
// 16-B vectors (plain loads and stores in program order of one lane: no fence, no barrier), laid out
// [slot][layer][tile][thread], so a wave instruction moves 1 KB contiguous.  A slot belongs to a
// workgroup of one launch, not to a (point, block) pair: a call runs as consecutive k_paths_gen
// launches of at most gen_slots(HCAP) blocks each on the call's stream, so the stash does not grow
// with n M.
//
// Head nets (NetGenHead): a construct_mlp net whose last Linear outputs grad_x u directly — ValueGradient
// (1 + nx outputs: u, grad u) or OnlyGradient (nx outputs: grad u; u = 0).  They need the forward pass
// only: no act' stash, no backward loop, so no slot ownership — a call is one k_paths_head launch over
// all its blocks.  The gradient block G (nx x H_last) of the last Linear is laid out as W1xT is, one
// row per state dimension, and feeds the same gen_stage + gen_dot loop with a_L as the B operand; Cha,
// which needs only sum_d u_x[d], takes it from cg = sum_d G[d] instead (two dots, no output GEMM).
//
// Terminal-enforcing nets (TERMA = true; the reference's PicardSolutionEnforceTerminal): the same two
// images, read as the hard-constraint ansatz u = g + (T - s) N (a value net) or
// grad u = grad g + (T - s) (G a_L + bg), u = 0 (an OnlyGradient head).  After the network phase every
// path takes g(X_s) and grad g(X_s) from one pass over its state dimensions (term_g); kernels of their
// own (k_paths_term, k_paths_head_term, k_baseline_term, k_baseline_head_term), so the existing ones
// keep their registers.
#pragma once

namespace dpi {

constexpr int GEN_LMAX = 8;    // hidden layers
constexpr int GEN_HMAX = 256;  // hidden width
// Most workgroups of one general path launch = stash slots: the resident workgroups of the 256 CUs
// (one per CU at HCAP = 256, whose LDS is 90 KB; two at HCAP = 128).
constexpr int gen_wgs(int hcap) { return hcap > 128 ? 1 : 2; }
constexpr int gen_slots(int hcap) { return 256 * gen_wgs(hcap); }

// Device image of a general net: every matrix fp32 row-major with row stride H = HCAP (128 or 256),
// zero-padded; a padded unit has zero weights in and out, so it adds exact zeros.
struct NetGen {
  int H;    // HCAP: the width cap of the instance and the row stride of the images
  int L;    // hidden layers, 1..GEN_LMAX
  int nxp;  // nx padded to 16
  int act;  // DPI_ACT_* of every hidden layer
  int ht;   // 16-unit tiles in use: the widest layer rounded up to 32, over 16 (even, <= H / 16)
  const float* W1x;   // (H, nxp)            W1[:, 1:]
  const float* w1t;   // (H)                 W1[:, 0]
  const float* b1;    // (H)
  const float* c1;    // (H)                 sum_d W1[h, 1 + d]
  const float* W1xT;  // (nxp up to 32, H)
  const float* W[GEN_LMAX];   // (H, H) hidden layer l = 1..L-1
  const float* WT[GEN_LMAX];
  const float* b[GEN_LMAX];
  const float* wout;  // (H)
  float bout;
};
// A head net's image: NetGen's (the baseline's forward pass reads the transposed images), with the last
// Linear split into the value row (wout, bout; ValueGradient only) and the gradient block.  c1 holds
// cg[h] = sum_d G[d][h] (formed in fp64 at upload, as a value net's c1 is).
struct NetGenHead : NetGen {
  int value;        // 1: ValueGradient, u = wout . a_L + bout; 0: OnlyGradient, u = 0
  const float* G;   // (nxp up to 32, H)   rows 1.. (ValueGradient) or 0.. (OnlyGradient) of the last Linear
  const float* bg;  // (nxp up to 32)      their biases
  float bgsum;      // sum_d bg[d]
};
// floats of one stash slot: act'(a_l) of layers 0..L-2, ht tiles of NTH float4 each
__host__ __device__ constexpr size_t gen_slot_floats(int L, int ht) { return (size_t)(L - 1) * ht * NTH * 4; }

// LDS of the general path kernel: the noise tile for nx <= 128, a 32-row fp32 weight stage of stride
// HCAP + 8 words (= 8 mod 16: the 16 rows x 4 column groups of a ds_read_b128 hit distinct banks),
// vec (base0 | w1t | wout | c1) and the biases of up to GEN_LMAX layers.  HCAP = 256: 90,368 B;
// HCAP = 128: 67,840 B.
template <int HCAP>
struct LdsGen {
  static constexpr int NXW = NXP_MAX;
  static constexpr int WS = HCAP + 8;
  float S[NXP_MAX * SS];
  float W[32 * WS];
  float vec[4 * HCAP];
  float bh[GEN_LMAX * HCAP];
  float xsh[NXP_MAX];
  float gst[4 * P * NSG];
  float tau[P], cmul[P], bsh[P];
};

// Rows [r0, r0 + 32) x columns [0, ncol) of a row-major global matrix of row stride ld into LDS rows of
// stride WS (ncol % 4 == 0).
template <int WS>
__device__ __forceinline__ void gen_stage(const float* __restrict__ g, int ld, int ncol, int r0, float* wsh) {
  const int nf4 = ncol >> 2;
  for (int idx = threadIdx.x; idx < 32 * nf4; idx += NTH) {
    const int r = idx / nf4, c = idx - r * nf4;
    *reinterpret_cast<float4*>(wsh + r * WS + 4 * c) = *reinterpret_cast<const float4*>(g + (size_t)(r0 + r) * ld + 4 * c);
  }
}
// One 16-row tile of (staged rows) x B over the first ht (even) column tiles; B in the C layout of
// the previous layer (unit 16 t + 4 qq + c of path jj), tiles >= ht hold zeros and are skipped.
template <int HT>
__device__ __forceinline__ floatx4 gen_dot(const float* wrow, const float (&b)[HT][4], int ht) {
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t0 = 0; t0 < HT; t0 += 2) {
    if (t0 < ht) {
#pragma unroll
      for (int t = t0; t < t0 + 2; ++t) {
        const float4 a = *reinterpret_cast<const float4*>(wrow + 16 * t);
        acc = mfma4(a.x, b[t][0], acc);
        acc = mfma4(a.y, b[t][1], acc);
        acc = mfma4(a.z, b[t][2], acc);
        acc = mfma4(a.w, b[t][3], acc);
      }
    }
  }
  return acc;
}

// Sums of fp64 statistics over the 4 lane groups of the MFMA C layout (as qsum) and over a wave.
__device__ __forceinline__ double qsum_d(double v) {
  v += __shfl_xor(v, 32, 64);
  return v + __shfl_xor(v, 16, 64);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// The terminal ansatz's g at X_s[d] = xsh[d] + cm S[d][pp] of path pp: the four lane groups split the
// dimensions (d = qq, qq + 4, ...) and are joined as qsum joins them.  Cha: returns g; grad_d g =
// k' g (1 - g) for every d.  OU: returns g = -log p_GMM and leaves the responsibilities r_c in rc
// (Eq<OU>::gstat_d / gfin_w: fp64 statistics); grad_d g = sum_c r_c (X_d - mean_cd) ivar_cd (term_dg).
// Reached by every lane of the workgroup: the loop bounds differ per lane group, the joins do not.
template <int KIND, int HCAP>
__device__ __forceinline__ float term_g(const EqDev& e, const LdsGen<HCAP>& sh, int pp, int qq, float cm,
                                        float (&rc)[NSG]) {
  if constexpr (!Eq<KIND>::GRAD_FULL) {
    float st[NSG];  // Cha: sum_d X_d in st[0]
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = rc[c] = 0.f;
    for (int d = qq; d < e.nx; d += 4) Eq<KIND>::gstat(e, d, fmaf(cm, sh.S[d * SS + pp], sh.xsh[d]), st);
    st[0] = qsum(st[0]);
    return Eq<KIND>::gfin(e, st);
  } else {
    double st[NSG];
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = 0.0;
    for (int d = qq; d < e.nx; d += 4) Eq<KIND>::gstat_d(e, d, fmaf(cm, sh.S[d * SS + pp], sh.xsh[d]), st);
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = qsum_d(st[c]);
    return Eq<KIND>::gfin_w(e, st, rc);
  }
}
// grad_d g of the OU mixture at X (the state's dimension d) from the responsibilities
__device__ __forceinline__ float term_dg(const EqDev& e, int d, float X, const float (&rc)[NSG]) {
  float z = 0.f;
#pragma unroll
  for (int c = 0; c < NSG; ++c)
    if (c < e.ncomp) z = fmaf(rc[c] * (X - e.mean[c * e.nx + d]), e.ivar[c * e.nx + d], z);
  return z;
}

// mlp_tile for a general net: same inputs (S tile, xsh, tau, cmul, vec, bh in LDS), outputs and tile
// orientation (hidden x path, wave = 16 paths, exact-fp32 v_mfma_f32_16x16x4_f32).  stash: this
// workgroup's slot.
// NET = NetGenHead: u and grad u are output columns (sh.bh[0 .. nxp) holds bg); stash is unused.
// TERMA: the terminal ansatz around the net's outputs; sh.bsh[pp] holds T - s of path pp on entry (the
// caller overwrites it after the call, from this wave).
template <int KIND, int HCAP, int ACT, class NET, bool TERMA = false>
__device__ __forceinline__ void mlp_tile_gen(const EqDev& e, const NET& net, LdsGen<HCAP>& sh, floatx4* stash,
                                             float& u_out, float& gsum_out, float& gA_out, float& gB_out) {
  constexpr bool HEAD = std::is_same_v<NET, NetGenHead>;
  constexpr int HT = HCAP / 16, WS = LdsGen<HCAP>::WS, H = HCAP;
  static_assert(HT % 2 == 0, "tiles are taken in pairs");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int jj = lane & 15, qq = lane >> 4;
  const int pp = 16 * wv + jj;
  const float tau = sh.tau[pp];
  const float cm = sh.cmul[pp];
  const int L = net.L, ht = net.ht, nxt = net.nxp >> 4, ncol = 16 * ht;
  floatx4* const st = stash + threadIdx.x;
  float a0[HT][4], a1[HT][4];  // the layer being consumed / produced
#pragma unroll
  for (int T = 0; T < HT; ++T)
#pragma unroll
    for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r] = 0.f;
  const float* const wrow = sh.W + jj * WS + 4 * qq;

  // ---------------- layer 1: z = base0 + w1t*tau + cmul * (W1x S)
#pragma unroll
  for (int T0 = 0; T0 < HT; T0 += 2) {
    if (T0 < ht) {
      __syncthreads();
      gen_stage<WS>(net.W1x, net.nxp, net.nxp, 16 * T0, sh.W);
      __syncthreads();
#pragma unroll
      for (int T2 = 0; T2 < 2; ++T2) {
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < nxt; ++t) {
          const float4 a = *reinterpret_cast<const float4*>(wrow + 16 * T2 * WS + 16 * t);
          const float* bc = sh.S + (16 * t + 4 * qq) * SS + pp;
          acc = mfma4(a.x, bc[0], acc);
          acc = mfma4(a.y, bc[SS], acc);
          acc = mfma4(a.z, bc[2 * SS], acc);
          acc = mfma4(a.w, bc[3 * SS], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int h = 16 * (T0 + T2) + 4 * qq + r;
          a0[T0 + T2][r] = Act<ACT>::f(fmaf(cm, acc[r], fmaf(sh.vec[H + h], tau, sh.vec[h])));
        }
      }
    }
  }
  // ---------------- hidden layers; act'(a_l) of every layer but the last goes to the stash
#pragma unroll 1
  for (int l = 1; l < L; ++l) {
    if constexpr (!HEAD) {
#pragma unroll
      for (int T = 0; T < HT; ++T)
        if (T < ht)
          st[((l - 1) * ht + T) * NTH] = floatx4{Act<ACT>::d(a0[T][0]), Act<ACT>::d(a0[T][1]), Act<ACT>::d(a0[T][2]),
                                                 Act<ACT>::d(a0[T][3])};
    }
    const float* const Wl = net.W[l];
    const float* const bl = sh.bh + l * H;
#pragma unroll
    for (int T0 = 0; T0 < HT; T0 += 2) {
      if (T0 < ht) {
        __syncthreads();
        gen_stage<WS>(Wl, H, ncol, 16 * T0, sh.W);
        __syncthreads();
#pragma unroll
        for (int T2 = 0; T2 < 2; ++T2) {
          const floatx4 acc = gen_dot<HT>(wrow + 16 * T2 * WS, a0, ht);
#pragma unroll
          for (int r = 0; r < 4; ++r) a1[T0 + T2][r] = Act<ACT>::f(acc[r] + bl[16 * (T0 + T2) + 4 * qq + r]);
        }
      }
    }
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r];
  }
  if constexpr (HEAD) {
    // ---------------- head: u = wout . a_L + bout (ValueGradient), grad u = G a_L + bg
    float up = 0.f, gp = 0.f;
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = 16 * T + 4 * qq + r;
        up = fmaf(sh.vec[2 * H + h], a0[T][r], up);
        if (!Eq<KIND>::GRAD_FULL) gp = fmaf(sh.vec[3 * H + h], a0[T][r], gp);
      }
    u_out = net.value ? qsum(up) + net.bout : 0.f;
    [[maybe_unused]] float tms = 0.f, rc[NSG];
    if constexpr (TERMA) {  // an OnlyGradient head: u = 0, grad u = grad g + (T - s) (G a_L + bg)
      tms = sh.bsh[pp];
      const float g = term_g<KIND>(e, sh, pp, qq, cm, rc);
      u_out = 0.f;
      if (!Eq<KIND>::GRAD_FULL) {
        gsum_out = fmaf(tms, qsum(gp) + net.bgsum, (float)e.nx * (e.cha_k * g * (1.0f - g)));
        gA_out = gB_out = 0.f;
        return;
      }
    }
    if (!Eq<KIND>::GRAD_FULL) {  // sum_d u_x[d] = cg . a_L + sum_d bg[d]
      gsum_out = qsum(gp) + net.bgsum;
      gA_out = gB_out = 0.f;
    } else {
      float A = 0.f, B = 0.f;
#pragma unroll 1
      for (int T0 = 0; T0 < nxt; T0 += 2) {
        __syncthreads();
        gen_stage<WS>(net.G, H, ncol, 16 * T0, sh.W);  // G has nxp rounded up to 32 rows
        __syncthreads();
#pragma unroll
        for (int T2 = 0; T2 < 2; ++T2) {
          const floatx4 acc = gen_dot<HT>(wrow + 16 * T2 * WS, a0, ht);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int d = 16 * (T0 + T2) + 4 * qq + r;
            if (d < e.nx) {
              const float X = fmaf(cm, sh.S[d * SS + pp], sh.xsh[d]);
              float z = acc[r] + sh.bh[d];
              if constexpr (TERMA) z = fmaf(tms, z, term_dg(e, d, X, rc));
              Eq<KIND>::gacc(e, d, X, z, A, B);
            }
          }
        }
      }
      gA_out = qsum(A);
      gB_out = qsum(B);
      gsum_out = 0.f;
    }
    return;
  }
  // ---------------- output u = wout . a_L + bout ; delta_L = wout * act'(a_L)
  float up = 0.f;
#pragma unroll
  for (int T = 0; T < HT; ++T)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = sh.vec[2 * H + 16 * T + 4 * qq + r];
      up = fmaf(w, a0[T][r], up);
      a0[T][r] = w * Act<ACT>::d(a0[T][r]);
    }
  u_out = qsum(up) + net.bout;
  [[maybe_unused]] float tms = 0.f, gterm = 0.f, rc[NSG];
  // ---------------- backward: delta_l = (W_{l+1}^T delta_{l+1}) * act'(a_l)
#pragma unroll 1
  for (int l = L - 2; l >= 0; --l) {
    const float* const Wt = net.WT[l + 1];
#pragma unroll
    for (int T0 = 0; T0 < HT; T0 += 2) {
      if (T0 < ht) {
        __syncthreads();
        gen_stage<WS>(Wt, H, ncol, 16 * T0, sh.W);
        __syncthreads();
#pragma unroll
        for (int T2 = 0; T2 < 2; ++T2) {
          const floatx4 acc = gen_dot<HT>(wrow + 16 * T2 * WS, a0, ht);
          const floatx4 d = st[(l * ht + T0 + T2) * NTH];
#pragma unroll
          for (int r = 0; r < 4; ++r) a1[T0 + T2][r] = acc[r] * d[r];
        }
      }
    }
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r];
  }
  if constexpr (TERMA) {  // u = g + (T - s) N, grad u = grad g + (T - s) grad N
    tms = sh.bsh[pp];
    gterm = term_g<KIND>(e, sh, pp, qq, cm, rc);
    u_out = fmaf(tms, u_out, gterm);
  }
  // ---------------- input gradient
  if (!Eq<KIND>::GRAD_FULL) {
    float gp = 0.f;
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) gp = fmaf(sh.vec[3 * H + 16 * T + 4 * qq + r], a0[T][r], gp);
    gsum_out = qsum(gp);
    if constexpr (TERMA) gsum_out = fmaf(tms, gsum_out, (float)e.nx * (e.cha_k * gterm * (1.0f - gterm)));
    gA_out = gB_out = 0.f;
  } else {
    float A = 0.f, B = 0.f;
#pragma unroll 1
    for (int T0 = 0; T0 < nxt; T0 += 2) {
      __syncthreads();
      gen_stage<WS>(net.W1xT, H, ncol, 16 * T0, sh.W);  // W1xT has nxp rounded up to 32 rows
      __syncthreads();
#pragma unroll
      for (int T2 = 0; T2 < 2; ++T2) {
        const floatx4 acc = gen_dot<HT>(wrow + 16 * T2 * WS, a0, ht);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * (T0 + T2) + 4 * qq + r;
          if (d < e.nx) {
            const float X = fmaf(cm, sh.S[d * SS + pp], sh.xsh[d]);
            float z = acc[r];
            if constexpr (TERMA) z = fmaf(tms, z, term_dg(e, d, X, rc));
            Eq<KIND>::gacc(e, d, X, z, A, B);
          }
        }
      }
    }
    gA_out = qsum(A);
    gB_out = qsum(B);
    gsum_out = 0.f;
  }
}

// ------------------------------------------------------------------------------ baseline
// base_point for a general net (HCAP <= GEN_HMAX, L <= GEN_LMAX): the same gx, fb and bx[n][HCAP],
// sampling (smp) and ticket zeroing; one thread per hidden unit, mat-vecs over the transposed images
// (coalesced in the unit), in a fixed order.
struct BaseLdsGen {
  float xs[NXP_MAX];
  float act[GEN_LMAX][GEN_HMAX];
  float dbuf[2][GEN_HMAX];
  float red[NTB / 64];
  float redn[NTB / 64][NSG];
  float ts;
};
// y[tid] = sum_k Wt[k][tid] v[k], k < K, tid < H (row stride H)
__device__ __forceinline__ float gen_matvec(const float* __restrict__ Wt, const float* v, int K, int H) {
  const int tid = threadIdx.x;
  float y0 = 0.f, y1 = 0.f;
  if (tid < H) {
    int k = 0;
    for (; k + 1 < K; k += 2) {
      y0 = fmaf(Wt[(size_t)k * H + tid], v[k], y0);
      y1 = fmaf(Wt[(size_t)(k + 1) * H + tid], v[k + 1], y1);
    }
    if (k < K) y0 = fmaf(Wt[(size_t)k * H + tid], v[k], y0);
  }
  return y0 + y1;
}
// NET = NetGenHead (k_baseline_head): u and grad u at the point itself from the output columns.
// TERMA: the terminal ansatz at the point, u = g(x) + (T - t) N and grad g(x) + (T - t) grad N (a head:
// its gradient rows, u = 0); thread 0 leaves g(x) in redn[0][0] and the OU responsibilities (from fp64
// statistics of their own) in redn[1], which nobody reads after the g(x) reduction, and the first layer's
// barrier publishes them.
template <int KIND, class NET, bool TERMA = false>
__device__ __forceinline__ void baseline_gen_body(const EqDev& e, const NET& net, const float* __restrict__ tx, int n,
                                                  float* __restrict__ gx, float* __restrict__ fb,
                                                  float* __restrict__ bx, const SampleSpec& smp,
                                                  int* __restrict__ tickets) {
  constexpr bool HEAD = std::is_same_v<NET, NetGenHead>;
  static_assert(KIND != DPI_EQ_GBM, "the general family: Cha / OU");
  static_assert(NTB >= GEN_HMAX && NTB >= NXP_MAX, "one thread per hidden unit and per state dimension");
  constexpr int NT = NTB;
  __shared__ BaseLdsGen bs;
  (void)n;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int nx = e.nx, F = 1 + nx;
  if (tickets && tid == 0) tickets[i] = 0;
  if (smp.tx) {  // base_point's draws
    const uint32_t ig = smp.point_base + (uint32_t)i;
    const int nb = (nx + 3) >> 2;
    float* row = smp.tx + (size_t)i * F;
    if (tid < nb) {
      const float tt = sample_point_t(e, smp, ig);
      if (tid == 0) {
        row[0] = tt;
        bs.ts = tt;
      }
      float x[4];
      sample_point_x4<KIND>(e, smp, ig, tid, tt, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int d = 4 * tid + q;
        if (d < nx) row[1 + d] = x[q];
        bs.xs[d] = d < nx ? x[q] : 0.f;
      }
    } else if (4 * nb <= tid && tid < NXP_MAX) {
      bs.xs[tid] = 0.f;
    }
  } else {
    const float* row = tx + (size_t)i * F;
    if (tid == 0) bs.ts = row[0];
    if (tid < NXP_MAX) bs.xs[tid] = tid < nx ? row[1 + tid] : 0.f;
  }
  __syncthreads();
  const float t = bs.ts;
  {  // g(x)
    float st[NSG];
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = 0.f;
    for (int d = tid; d < nx; d += NT) Eq<KIND>::gstat(e, d, bs.xs[d], st);
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = wave_sum(st[c]);
    if ((tid & 63) == 0)
#pragma unroll
      for (int c = 0; c < NSG; ++c) bs.redn[tid >> 6][c] = st[c];
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < NSG; ++c) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) a += bs.redn[w][c];
        st[c] = a;
      }
      const float g = Eq<KIND>::gfin(e, st);
      gx[i] = g;
      if constexpr (TERMA && !Eq<KIND>::GRAD_FULL) bs.redn[0][0] = g;
    }
  }
  if constexpr (TERMA && Eq<KIND>::GRAD_FULL) {  // g(x) and the responsibilities from fp64 statistics (gfin_w)
    static_assert(NT / 64 >= 2, "redn[1] holds the responsibilities");
    __shared__ double redd[NT / 64][NSG];
    double sd[NSG];
#pragma unroll
    for (int c = 0; c < NSG; ++c) sd[c] = 0.0;
    for (int d = tid; d < nx; d += NT) Eq<KIND>::gstat_d(e, d, bs.xs[d], sd);
#pragma unroll
    for (int c = 0; c < NSG; ++c) sd[c] = wave_sum_d(sd[c]);
    if ((tid & 63) == 0)
#pragma unroll
      for (int c = 0; c < NSG; ++c) redd[tid >> 6][c] = sd[c];
    __syncthreads();  // thread 0 is past its reads of redn
    if (tid == 0) {
      float rc[NSG];
#pragma unroll
      for (int c = 0; c < NSG; ++c) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) a += redd[w][c];
        sd[c] = a;
      }
      bs.redn[0][0] = Eq<KIND>::gfin_w(e, sd, rc);
#pragma unroll
      for (int c = 0; c < NSG; ++c) bs.redn[1][c] = rc[c];
    }
  }
  const int H = net.H, L = net.L, nxp = net.nxp, hu = 16 * net.ht;  // hu: units in use
  {
    const float acc = gen_matvec(net.W1xT, bs.xs, nx, H);
    if (tid < H) {
      const float v = net.b1[tid] + acc;
      bx[(size_t)i * H + tid] = v;
      bs.act[0][tid] = act_f(net.act, fmaf(net.w1t[tid], t, v));
    }
    __syncthreads();
  }
  for (int l = 1; l < L; ++l) {
    const float acc = gen_matvec(net.WT[l], bs.act[l - 1], hu, H);
    if (tid < H) bs.act[l][tid] = act_f(net.act, acc + net.b[l][tid]);
    __syncthreads();
  }
  // the ansatz's factors (the layers' barriers published redn)
  [[maybe_unused]] float tmt = 0.f, gterm = 0.f, rc[NSG];
  if constexpr (TERMA) {
    tmt = e.T - t;
    gterm = bs.redn[0][0];
#pragma unroll
    for (int c = 0; c < NSG; ++c) rc[c] = Eq<KIND>::GRAD_FULL ? bs.redn[1][c] : 0.f;
  }
  if constexpr (HEAD) {
    const float* const aL = bs.act[L - 1];
    float u = net.value ? block_sum_n<NT>(tid < H ? net.wout[tid] * aL[tid] : 0.f, bs.red) + net.bout : 0.f;
    if constexpr (TERMA) u = 0.f;
    float gs = 0.f, gA = 0.f, gB = 0.f;
    if (!Eq<KIND>::GRAD_FULL) {
      gs = block_sum_n<NT>(tid < H ? net.c1[tid] * aL[tid] : 0.f, bs.red) + net.bgsum;
      if constexpr (TERMA) gs = fmaf(tmt, gs, (float)nx * (e.cha_k * gterm * (1.0f - gterm)));
    } else {  // one wave per row of G (coalesced in the unit), rows in a fixed order
      float A = 0.f, B = 0.f;
      for (int d = tid >> 6; d < nx; d += NT / 64) {
        float z = 0.f;
        for (int k = tid & 63; k < hu; k += 64) z = fmaf(net.G[(size_t)d * H + k], aL[k], z);
        z = wave_sum(z);
        if ((tid & 63) == 0) {
          z += net.bg[d];
          if constexpr (TERMA) z = fmaf(tmt, z, term_dg(e, d, bs.xs[d], rc));
          Eq<KIND>::gacc(e, d, bs.xs[d], z, A, B);
        }
      }
      gA = block_sum_n<NT>(A, bs.red);
      gB = block_sum_n<NT>(B, bs.red);
    }
    if (tid == 0) fb[i] = Eq<KIND>::ffv(e, u, gs, gA, gB);
    return;
  }
  float u = block_sum_n<NT>(tid < H ? net.wout[tid] * bs.act[L - 1][tid] : 0.f, bs.red) + net.bout;
  if constexpr (TERMA) u = fmaf(tmt, u, gterm);
  int cur = 0;
  if (tid < H) bs.dbuf[0][tid] = net.wout[tid] * act_d(net.act, bs.act[L - 1][tid]);
  __syncthreads();
  for (int l = L - 2; l >= 0; --l) {
    const float acc = gen_matvec(net.W[l + 1], bs.dbuf[cur], hu, H);
    if (tid < H) bs.dbuf[cur ^ 1][tid] = acc * act_d(net.act, bs.act[l][tid]);
    cur ^= 1;
    __syncthreads();
  }
  float gs = 0.f, gA = 0.f, gB = 0.f;
  if (!Eq<KIND>::GRAD_FULL) {
    gs = block_sum_n<NT>(tid < H ? net.c1[tid] * bs.dbuf[cur][tid] : 0.f, bs.red);
    if constexpr (TERMA) gs = fmaf(tmt, gs, (float)nx * (e.cha_k * gterm * (1.0f - gterm)));
  } else {
    float A = 0.f, B = 0.f;
    for (int d = tid; d < nx; d += NT) {
      float z = 0.f;
      for (int k = 0; k < hu; ++k) z = fmaf(net.W1x[(size_t)k * nxp + d], bs.dbuf[cur][k], z);
      if constexpr (TERMA) z = fmaf(tmt, z, term_dg(e, d, bs.xs[d], rc));
      Eq<KIND>::gacc(e, d, bs.xs[d], z, A, B);
    }
    gA = block_sum_n<NT>(A, bs.red);
    gB = block_sum_n<NT>(B, bs.red);
  }
  if (tid == 0) fb[i] = Eq<KIND>::ffv(e, u, gs, gA, gB);  // state-dependent part
}
template <int KIND>
__global__ __launch_bounds__(NTB) void k_baseline_gen(EqDev e, NetGen net, const float* __restrict__ tx, int n,
                                                     float* __restrict__ gx, float* __restrict__ fb,
                                                     float* __restrict__ bx, SampleSpec smp, int* __restrict__ tickets) {
  baseline_gen_body<KIND>(e, net, tx, n, gx, fb, bx, smp, tickets);
}
template <int KIND>
__global__ __launch_bounds__(NTB) void k_baseline_head(EqDev e, NetGenHead net, const float* __restrict__ tx, int n,
                                                      float* __restrict__ gx, float* __restrict__ fb,
                                                      float* __restrict__ bx, SampleSpec smp, int* __restrict__ tickets) {
  baseline_gen_body<KIND>(e, net, tx, n, gx, fb, bx, smp, tickets);
}
// The terminal-enforcing forms (TERMA): kernels of their own.
template <int KIND>
__global__ __launch_bounds__(NTB) void k_baseline_term(EqDev e, NetGen net, const float* __restrict__ tx, int n,
                                                      float* __restrict__ gx, float* __restrict__ fb,
                                                      float* __restrict__ bx, SampleSpec smp, int* __restrict__ tickets) {
  baseline_gen_body<KIND, NetGen, true>(e, net, tx, n, gx, fb, bx, smp, tickets);
}
template <int KIND>
__global__ __launch_bounds__(NTB) void k_baseline_head_term(EqDev e, NetGenHead net, const float* __restrict__ tx,
                                                           int n, float* __restrict__ gx, float* __restrict__ fb,
                                                           float* __restrict__ bx, SampleSpec smp,
                                                           int* __restrict__ tickets) {
  baseline_gen_body<KIND, NetGenHead, true>(e, net, tx, n, gx, fb, bx, smp, tickets);
}

}  // namespace dpi
