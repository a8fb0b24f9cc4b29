// The general MLP family for GBM (GBMEquationComplexExact, nx <= 128): any construct_mlp value network of
// 1..GEN_LMAX hidden layers, each 1..GG_H = 64 wide, all-ELU or all-Tanh, that has no specialised GBM
// k_paths instance (dpi_route.h DPI_SHAPES_GBM).  Included by dpi_device.h after dpi_general.h.
//
// The net is read from the NetGen image of width cap 128 that the upload already builds (row stride
// net.H = 128, ht = 2 or 4 tiles in use); nothing is uploaded twice.
//
// Phase 2 is mlp_hdiag's contract, s1 = sum_d cnt[d] u_dd and s2 = sum_d cnt[d] |u_dd|, computed the same
// way: one forward pass, one adjoint pass for lam_l = du/da_l, then first-order tangents per direction,
// u_dd = sum_l <lam_l act''(a_l), (dz_l/dx_d)^2>, all on the exact-fp32 v_mfma_f32_16x16x4_f32 in the
// hidden x path orientation, one wave owning 16 paths.
//
// Where the per-layer state lives.  The sweep needs p_l = act'(a_l) (l < L - 1) and q_l = lam_l act''(a_l)
// (every l) for every direction: 2 L x 4 tiles x 4 values per lane, 256 at L = 8.  Registers would hold
// them only with a static layer index, i.e. L as a template argument: 8 depths x 2 activations of a fully
// unrolled 512-register kernel.  LDS cannot: 2 x 64 x 64 x 4 B = 32 KB per layer.  So the layer loop is a
// run-time loop and the state is parked in the general family's stash, as mlp_tile_gen parks act': every
// lane writes and re-reads its own 16-B fragments, [layer][tile][thread], no fence or barrier.  q_0 stays
// in registers, so a slot is 2 (L - 1) ht float4 per thread and the 256 slots of this kernel (one
// workgroup per CU) fill exactly the stash region a net of these shapes already has (512 slots of
// (L - 1) ht): the workspace does not change.  The re-reads are amortised over a batch of GG_DB = 4
// directions: per batch and layer a lane reads 2 x 4 x 16 B, 100 directions x 8 layers = 25.6 KB per
// lane per block, against 64 MFMAs per direction and layer.
//
// Where the weights live.  W1x (34 KB at nx = 128) is LDS-resident: layer 0's A operand and the sweep's
// z_0 = W1x[:, d], four directions per 16-B read.  The hidden matrices (L - 1 <= 7 of 64 x 64, 18 KB
// padded) do not fit beside it and the 34 KB noise tile, so they are staged through two LDS buffers: with
// L - 1 <= 2 both stay resident; otherwise, while the waves run a layer's MFMAs for the batch out of one
// buffer, every thread holds the next layer's 4 float4 in registers, then writes them to the other buffer
// and the workgroup meets at ONE barrier per (batch, layer) step.
//
// A path's result does not depend on its neighbours: every direction is its own MFMA column chain, summed
// into s1 / s2 in increasing d; the last batch's slots past nx read the image's zero columns and a zero
// count: fmaf(0, 0, s).
#pragma once

namespace dpi {

constexpr int GG_H = 64;       // width cap
constexpr int GG_DB = 4;       // directions per batch of the sweep
constexpr int GG_SLOTS = 256;  // most workgroups of one launch = stash slots (one workgroup per CU)
// float4 of one stash slot: p_0..p_{L-2} then q_1..q_{L-1}, ht tiles of NTH each
__host__ __device__ constexpr size_t gg_slot_vec4(int L, int ht) { return (size_t)2 * (L - 1) * ht * NTH; }
static_assert(GG_SLOTS * 2 == gen_slots(128), "the slots fill the stash region of the width-128 general image");

struct LdsGbmGen {
  static constexpr int NXW = NXP_MAX;
  static constexpr int WXS = NXP_MAX + 8;  // W1x row stride (as LdsGbm)
  static constexpr int WHS = GG_H + 8;     // hidden row stride
  __attribute__((aligned(16))) float S[NXP_MAX * SS];
  float W1x[GG_H * WXS];
  float Wh[2][GG_H * WHS];
  float vec[4 * GG_H];
  float bh[GEN_LMAX * GG_H];
  float xsh[NXP_MAX];
  float hb[NXP_MAX];
  float gst[4 * P * NSG];
  float fst[4 * P * NSG];
  float wx[NSG];
  float tau[P], cmul[P], bsh[P], fbp[P];
  unsigned char cnt[NXP_MAX * P];  // SDGD index histogram [d][path]
};

// The 16 ht x 16 ht block of a row-major global matrix of row stride ld, as 16-B pieces: piece k of this
// thread (k < 4; 16 ht x 4 ht <= 1024 pieces).
__device__ __forceinline__ void gg_fetch(const float* __restrict__ g, int ld, int ht, float4 (&pf)[4]) {
  const int nf4 = 4 * ht, tot = 16 * ht * nf4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = threadIdx.x + k * NTH, r = idx / nf4, c = idx - r * nf4;
    pf[k] = idx < tot ? *reinterpret_cast<const float4*>(g + (size_t)r * ld + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ void gg_put(const float4 (&pf)[4], int ht, float* wsh) {
  const int nf4 = 4 * ht, tot = 16 * ht * nf4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = threadIdx.x + k * NTH, r = idx / nf4, c = idx - r * nf4;
    if (idx < tot) *reinterpret_cast<float4*>(wsh + r * LdsGbmGen::WHS + 4 * c) = pf[k];
  }
}
__device__ __forceinline__ void gg_stage(const float* __restrict__ g, int ld, int ht, float* wsh) {
  float4 pf[4];
  gg_fetch(g, ld, ht, pf);
  gg_put(pf, ht, wsh);
}
// Row tile T of (staged matrix) x B; wrow = buffer + jj * WHS + 4 qq; tiles >= ht hold zeros and are skipped.
__device__ __forceinline__ floatx4 gg_dot(const float* wrow, int T, const float (&b)[GG_H / 16][4], int ht) {
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < GG_H / 16; ++t) {
    if (t < ht) {
      const float4 a = *reinterpret_cast<const float4*>(wrow + 16 * T * LdsGbmGen::WHS + 16 * t);
      acc = mfma4(a.x, b[t][0], acc);
      acc = mfma4(a.y, b[t][1], acc);
      acc = mfma4(a.z, b[t][2], acc);
      acc = mfma4(a.w, b[t][3], acc);
    }
  }
  return acc;
}

// mlp_hdiag for a general net: same inputs (S tile, W1x, cnt, xsh, tau, cmul, vec, bh in LDS) and outputs.
// stash: this workgroup's slot.  Reached by every wave of the workgroup (barriers inside).
template <int ACT>
__device__ __forceinline__ void mlp_hdiag_gen(const EqDev& e, const NetGen& net, LdsGbmGen& sh, floatx4* stash,
                                              float& s1_out, float& s2_out) {
  constexpr int H = GG_H, HT = GG_H / 16, WHS = LdsGbmGen::WHS, WXS = LdsGbmGen::WXS, DB = GG_DB;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int jj = lane & 15, qq = lane >> 4;
  const int pp = 16 * wv + jj;
  const float tau = sh.tau[pp];
  const float cm = sh.cmul[pp];
  const int L = net.L, ht = net.ht, nxt = net.nxp >> 4, ld = net.H;
  floatx4* const stp = stash + threadIdx.x;                             // p_l at stp[(l ht + T) NTH]
  floatx4* const stq = stp + (size_t)(L - 1) * ht * NTH - (size_t)ht * NTH;  // q_l (l >= 1) at stq[(l ht + T) NTH]
  float a0[HT][4], a1[HT][4];
#pragma unroll
  for (int T = 0; T < HT; ++T)
#pragma unroll
    for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r] = 0.f;
  const float* const w0 = sh.Wh[0] + jj * WHS + 4 * qq;

  // ---------------- forward; a_l of every layer but the last goes to the stash (p_l's place)
#pragma unroll
  for (int T = 0; T < HT; ++T) {
    if (T < ht) {
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* wrow = sh.W1x + (16 * T + jj) * WXS + 4 * qq;
      for (int t = 0; t < nxt; ++t) {
        const float4 a = *reinterpret_cast<const float4*>(wrow + 16 * t);
        const float* bc = sh.S + (16 * t + 4 * qq) * SS + pp;
        acc = mfma4(a.x, bc[0], acc);
        acc = mfma4(a.y, bc[SS], acc);
        acc = mfma4(a.z, bc[2 * SS], acc);
        acc = mfma4(a.w, bc[3 * SS], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = 16 * T + 4 * qq + r;
        a0[T][r] = Act<ACT>::f(fmaf(cm, acc[r], fmaf(sh.vec[H + h], tau, sh.vec[h])));
      }
    }
  }
#pragma unroll 1
  for (int l = 1; l < L; ++l) {
#pragma unroll
    for (int T = 0; T < HT; ++T)
      if (T < ht) stp[((l - 1) * ht + T) * NTH] = floatx4{a0[T][0], a0[T][1], a0[T][2], a0[T][3]};
    __syncthreads();
    gg_stage(net.W[l], ld, ht, sh.Wh[0]);
    __syncthreads();
    const float* const bl = sh.bh + l * H;
#pragma unroll
    for (int T = 0; T < HT; ++T) {
      if (T < ht) {
        const floatx4 acc = gg_dot(w0, T, a0, ht);
#pragma unroll
        for (int r = 0; r < 4; ++r) a1[T][r] = Act<ACT>::f(acc[r] + bl[16 * T + 4 * qq + r]);
      }
    }
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r];
  }
  // ---------------- adjoints lam_l = du/da_l; p_l = act'(a_l) and q_l = lam_l act''(a_l) replace a_l
  float q0[HT][4];
#pragma unroll
  for (int T = 0; T < HT; ++T) {
    float qv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = sh.vec[2 * H + 16 * T + 4 * qq + r], a = a0[T][r];
      qv[r] = w * Act<ACT>::d2(a);
      q0[T][r] = qv[r];
      a0[T][r] = w * Act<ACT>::d(a);
    }
    if (L > 1 && T < ht) stq[((L - 1) * ht + T) * NTH] = floatx4{qv[0], qv[1], qv[2], qv[3]};
  }
#pragma unroll 1
  for (int l = L - 2; l >= 0; --l) {
    __syncthreads();
    gg_stage(net.WT[l + 1], ld, ht, sh.Wh[0]);
    __syncthreads();
#pragma unroll
    for (int T = 0; T < HT; ++T) {
      if (T < ht) {
        const floatx4 lam = gg_dot(w0, T, a0, ht);
        const floatx4 av = stp[(l * ht + T) * NTH];
        floatx4 dv, qv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dv[r] = Act<ACT>::d(av[r]);
          qv[r] = lam[r] * Act<ACT>::d2(av[r]);
          a1[T][r] = dv[r] * lam[r];
          q0[T][r] = qv[r];  // the last iteration's (l = 0) stays
        }
        stp[(l * ht + T) * NTH] = dv;
        if (l > 0) stq[(l * ht + T) * NTH] = qv;
      }
    }
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) a0[T][r] = a1[T][r];
  }
  // ---------------- tangent sweep over the state dimensions, GG_DB directions per batch
  const bool resident = L - 1 <= 2;
  if (L > 1) {
    __syncthreads();
    gg_stage(net.W[1], ld, ht, sh.Wh[0]);
    if (L == 3) gg_stage(net.W[2], ld, ht, sh.Wh[1]);
    __syncthreads();
  }
  int cur = 0;  // streamed: the buffer that holds the layer about to be consumed
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 1
  for (int d0 = 0; d0 < e.nx; d0 += DB) {
    float z[DB][HT][4], term[DB];
#pragma unroll
    for (int k = 0; k < DB; ++k) term[k] = 0.f;
#pragma unroll
    for (int T = 0; T < HT; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 w = *reinterpret_cast<const float4*>(sh.W1x + (16 * T + 4 * qq + r) * WXS + d0);
        const float zz[DB] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < DB; ++k) {
          z[k][T][r] = zz[k];
          term[k] = fmaf(q0[T][r], zz[k] * zz[k], term[k]);
        }
      }
#pragma unroll 1
    for (int l = 1; l < L; ++l) {
      float4 pf[4];
      if (!resident) gg_fetch(net.W[l == L - 1 ? 1 : l + 1], ld, ht, pf);
      const float* const wb = sh.Wh[resident ? l - 1 : cur] + jj * WHS + 4 * qq;
      floatx4 pv[HT], qv[HT];
#pragma unroll
      for (int T = 0; T < HT; ++T) {
        pv[T] = qv[T] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (T < ht) {
          pv[T] = stp[((l - 1) * ht + T) * NTH];
          qv[T] = stq[(l * ht + T) * NTH];
        }
      }
#pragma unroll
      for (int k = 0; k < DB; ++k)
#pragma unroll
        for (int T = 0; T < HT; ++T)
#pragma unroll
          for (int r = 0; r < 4; ++r) z[k][T][r] *= pv[T][r];
      float zn[DB][HT][4];
#pragma unroll
      for (int T = 0; T < HT; ++T) {
        floatx4 acc[DB];
#pragma unroll
        for (int k = 0; k < DB; ++k) acc[k] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (T < ht) {
#pragma unroll
          for (int t = 0; t < HT; ++t) {
            if (t < ht) {
              const float4 a = *reinterpret_cast<const float4*>(wb + 16 * T * WHS + 16 * t);
#pragma unroll
              for (int k = 0; k < DB; ++k) {
                acc[k] = mfma4(a.x, z[k][t][0], acc[k]);
                acc[k] = mfma4(a.y, z[k][t][1], acc[k]);
                acc[k] = mfma4(a.z, z[k][t][2], acc[k]);
                acc[k] = mfma4(a.w, z[k][t][3], acc[k]);
              }
            }
          }
        }
#pragma unroll
        for (int k = 0; k < DB; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            zn[k][T][r] = acc[k][r];
            term[k] = fmaf(qv[T][r], acc[k][r] * acc[k][r], term[k]);
          }
      }
#pragma unroll
      for (int k = 0; k < DB; ++k)
#pragma unroll
        for (int T = 0; T < HT; ++T)
#pragma unroll
          for (int r = 0; r < 4; ++r) z[k][T][r] = zn[k][T][r];
      if (!resident) {  // every wave is past the other buffer's reads (the previous step's barrier)
        gg_put(pf, ht, sh.Wh[cur ^ 1]);
        __syncthreads();
        cur ^= 1;
      }
    }
#pragma unroll
    for (int k = 0; k < DB; ++k) {
      const float ud = qsum(term[k]);
      const float c = (float)sh.cnt[(d0 + k) * P + pp];  // d0 + k < nxp: zero count and zero column past nx
      s1 = fmaf(c, ud, s1);
      s2 = fmaf(c, fabsf(ud), s2);
    }
  }
  s1_out = s1;
  s2_out = s2;
}

// ------------------------------------------------------------------------------ baseline
// k_baseline_gbm for a general net (widths <= GG_H, L <= GEN_LMAX; NetGen image, row stride net.H): g(x),
// the exact-solution part of ffi at (t, x), bx[n][GG_H] = b1 + W1[:, 1:] x and the network's Hessian
// diagonal hb[n][HBS] at (t, x); smp / tickets as k_baseline_gbm.  The same steps in the same orders; a
// kernel of its own, so k_baseline_gbm keeps its resources (a template, so only its unit defines it).
template <int HC>
__global__ __launch_bounds__(NTHB) void k_baseline_gbm_gen(EqDev e, NetGen net, const float* __restrict__ tx, int n,
                                                          float* __restrict__ gx, float* __restrict__ fb,
                                                          float* __restrict__ bx, float* __restrict__ hb, SampleSpec smp,
                                                          int* __restrict__ tickets) {
  constexpr int KIND = DPI_EQ_GBM;
  static_assert(HC == GG_H, "one instance: the family's width cap");
  __shared__ float xs[NXP_MAX];
  __shared__ float act[GEN_LMAX][HC];
  __shared__ float red[NTHB / 64];
  __shared__ float ts;
  (void)n;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int nx = e.nx, F = 1 + nx;
  if (tickets && tid == 0) tickets[i] = 0;
  if (smp.tx) {
    const uint32_t ig = smp.point_base + (uint32_t)i;
    const int nb = (nx + 3) >> 2;
    float* row = smp.tx + (size_t)i * F;
    if (tid < nb) {
      const float tt = sample_point_t(e, smp, ig);
      if (tid == 0) {
        row[0] = tt;
        ts = tt;
      }
      float x[4];
      sample_point_x4<KIND>(e, smp, ig, tid, tt, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int d = 4 * tid + q;
        if (d < nx) row[1 + d] = x[q];
        xs[d] = d < nx ? x[q] : 0.f;
      }
    } else if (4 * nb <= tid && tid < NXP_MAX) {
      xs[tid] = 0.f;
    }
  } else {
    const float* row = tx + (size_t)i * F;
    if (tid == 0) ts = row[0];
    if (tid < NXP_MAX) xs[tid] = tid < nx ? row[1 + tid] : 0.f;
  }
  __syncthreads();
  const float t = ts;
  {  // g(x)
    __shared__ float redn[NTHB / 64][NSG];
    float st[NSG];
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = 0.f;
    for (int d = tid; d < nx; d += NTHB) Eq<KIND>::gstat(e, d, xs[d], st);
#pragma unroll
    for (int c = 0; c < NSG; ++c) st[c] = wave_sum(st[c]);
    if ((tid & 63) == 0)
#pragma unroll
      for (int c = 0; c < NSG; ++c) redn[tid >> 6][c] = st[c];
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < NSG; ++c) {
        float a = 0.f;
        for (int w = 0; w < NTHB / 64; ++w) a += redn[w][c];
        st[c] = a;
      }
      gx[i] = Eq<KIND>::gfin(e, st);
    }
  }
  // exact-solution part of ffi at (t, x)
  float arg[NSG], sn[NSG];
  {
    __shared__ float redw[NTHB / 64][NSG];
    float v[NSG];
#pragma unroll
    for (int c = 0; c < NSG; ++c) {
      v[c] = 0.f;
      if (c < e.nodes)
        for (int d = tid; d < nx; d += NTHB) v[c] = fmaf(e.gw[c * F + 1 + d], xs[d], v[c]);
      v[c] = wave_sum(v[c]);
    }
    __syncthreads();
    if ((tid & 63) == 0)
#pragma unroll
      for (int c = 0; c < NSG; ++c) redw[tid >> 6][c] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NSG; ++c) {
      float a = 0.f;
      for (int w = 0; w < NTHB / 64; ++w) a += redw[w][c];
      arg[c] = c < e.nodes ? fmaf(e.gw[c * F], t, a) : 0.f;
      sn[c] = __sinf(arg[c]);
    }
  }
  const float ah = block_sum_n<NTHB>(Eq<KIND>::abs_hess_partial(e, sn, tid, NTHB), red);
  const float Cb = Eq<KIND>::exact_scalar_terms(e, arg) - 0.25f * ah;
  const int Hs = net.H, L = net.L, nxp = net.nxp, hu = 16 * net.ht;  // row stride; units in use (32 or 64)
  __shared__ __attribute__((aligned(16))) float part[NTHB / 64][HMAX];
  {
    const float acc = base_matvec<NTHB>(net.W1xT, xs, nx, Hs, part);
    if (tid < HC) {
      bx[(size_t)i * HC + tid] = net.b1[tid] + acc;
      act[0][tid] = act_f(net.act, fmaf(net.w1t[tid], t, net.b1[tid] + acc));
    }
    __syncthreads();
  }
  for (int l = 1; l < L; ++l) {
    const float acc = base_matvec<NTHB>(net.WT[l], act[l - 1], hu, Hs, part);
    if (tid < HC) act[l][tid] = act_f(net.act, acc + net.b[l][tid]);
    __syncthreads();
  }
  // adjoints lam_l = W_{l+1}^T (act'(a_{l+1}) * lam_{l+1})
  __shared__ float lamb[GEN_LMAX][HC];
  __shared__ float cb[HC];
  __shared__ __attribute__((aligned(16))) float ztb[2][HC][NXP_MAX];
  if (tid < HC) lamb[L - 1][tid] = net.wout[tid];
  __syncthreads();
  for (int l = L - 2; l >= 0; --l) {
    if (tid < HC) cb[tid] = act_d(net.act, act[l + 1][tid]) * lamb[l + 1][tid];
    __syncthreads();
    const float acc = base_matvec<NTHB>(net.W[l + 1], cb, hu, Hs, part);
    if (tid < HC) lamb[l][tid] = acc;
    __syncthreads();
  }
  // tangent sweep as an LDS mat-mat per layer (k_baseline_gbm's): thread t < 512 owns rows hg + 16 j and
  // columns 4 dg .. 4 dg + 3
  __shared__ __attribute__((aligned(16))) float wsc[HC * HC];
  __shared__ float udp[16][NXP_MAX];
  const bool sw = tid < 512;
  const int dg = tid & 31, hg = (tid >> 5) & 15, RJ = hu >> 4;
  float ud[4] = {0.f, 0.f, 0.f, 0.f};
  if (sw) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = hg + 16 * j;
      if (j < RJ) {
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int d = 4 * dg + q;
          z[q] = d < nx ? net.W1x[(size_t)h * nxp + d] : 0.f;
        }
        *reinterpret_cast<float4*>(&ztb[0][h][4 * dg]) = make_float4(z[0], z[1], z[2], z[3]);
        const float c = lamb[0][h] * act_d2(net.act, act[0][h]);
#pragma unroll
        for (int q = 0; q < 4; ++q) ud[q] = fmaf(c, z[q] * z[q], ud[q]);
      }
    }
  }
  int cz = 0;
  for (int l = 1; l < L; ++l) {
    for (int q = tid; q < hu * hu; q += NTHB) {
      const int h = q / hu, k = q - h * hu;
      wsc[h * HC + k] = net.W[l][(size_t)h * Hs + k] * act_d(net.act, act[l - 1][k]);
    }
    __syncthreads();  // wsc and Z_{l-1} complete
    if (sw) {
      float z[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) z[j][q] = 0.f;
#pragma unroll 1
      for (int k = 0; k < hu; k += 4) {
        const float4 z0 = *reinterpret_cast<const float4*>(&ztb[cz][k][4 * dg]);
        const float4 z1 = *reinterpret_cast<const float4*>(&ztb[cz][k + 1][4 * dg]);
        const float4 z2 = *reinterpret_cast<const float4*>(&ztb[cz][k + 2][4 * dg]);
        const float4 z3 = *reinterpret_cast<const float4*>(&ztb[cz][k + 3][4 * dg]);
        const float b0[4] = {z0.x, z0.y, z0.z, z0.w}, b1[4] = {z1.x, z1.y, z1.z, z1.w};
        const float b2[4] = {z2.x, z2.y, z2.z, z2.w}, b3[4] = {z3.x, z3.y, z3.z, z3.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < RJ) {
            const float4 w = *reinterpret_cast<const float4*>(&wsc[(hg + 16 * j) * HC + k]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              z[j][q] = fmaf(w.w, b3[q], fmaf(w.z, b2[q], fmaf(w.y, b1[q], fmaf(w.x, b0[q], z[j][q]))));
          }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int h = hg + 16 * j;
        if (j < RJ) {
          *reinterpret_cast<float4*>(&ztb[cz ^ 1][h][4 * dg]) = make_float4(z[j][0], z[j][1], z[j][2], z[j][3]);
          const float c = lamb[l][h] * act_d2(net.act, act[l][h]);
#pragma unroll
          for (int q = 0; q < 4; ++q) ud[q] = fmaf(c, z[j][q] * z[j][q], ud[q]);
        }
      }
    }
    cz ^= 1;
    __syncthreads();  // before wsc is overwritten
  }
  if (sw)
#pragma unroll
    for (int q = 0; q < 4; ++q) udp[hg][4 * dg + q] = ud[q];
  __syncthreads();
  if (tid < NXP_MAX) {
    float a = 0.f;
    for (int g = 0; g < 16; ++g) a += udp[g][tid];
    hb[(size_t)i * HBS + tid] = tid < nx ? a : 0.f;
  }
  if (tid == 0) fb[i] = Cb;
}

}  // namespace dpi
