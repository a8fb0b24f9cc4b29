// The shell of a PISGradNet fit on the device ("The PISGradNet shell"; TRAIN.PIS_SHELL: hip):
// everything fit._pis_objective forms around the core primitive of dpi_fit.h — the timestep embedding,
// t_encoder, smooth_net at lambda and at the zero point, the parameter-free g0 part, the loss, and the
// reverse pass of the two time networks down to the phase.
//
//   k_fit_shell_fwd       one workgroup per tile of 64 batch rows (lane = row, fit_mv's layout: the time networks
//                         are 64 wide, one unit pass per wave), and one more workgroup for the zero point of
//                         smoothing_function, which is a single evaluation: it runs smooth_net on lambda = 0 as the
//                         row behind the batch's tiles and parks its state there.  Writes tau, s, res, res_x.
//   k_fit_shell_loss      one workgroup per tile (lane = column, four waves over the tile's rows): u, u_x, the
//                         loss terms, the seeds e, r and sbar, and the tile's loss sums
//   k_fit_shell_loss_sum  one workgroup: the tiles' sums in tile order, `losses`
//   k_fit_shell_bwd       the reverse pass of t_encoder (from taubar) and of smooth_net (from sbar; the zero
//                         point's workgroup from -sum sbar) down to the cotangent of the embedding and of omega
//   k_fit_shell_wgrad     k_fit_core_wgrad's row walk over the parked state: every dW, db and d phase, the zero
//                         point's row last
//
// As in dpi_fit.h: exact fp32 VALU for the networks, fp64 for omega and its sine and cosine, for the statistics
// of g, for the residuals, loss terms and seeds (rounded once) and for every sum over rows, which runs in fixed
// order; no atomics, no workgroup waits on another, every output is overwritten.  Rows past B load zeros and
// are never stored.
#pragma once
#include "dpi_fit.h"

namespace dpi {

constexpr int SH_NT = CORE_NT;         // channels: the width of both time networks
constexpr int SH_NE = 2 * SH_NT;       // the embedding (sin, cos)
constexpr int SH_LMAX = CORE_LMAX;     // smooth_net's 64 -> 64 layers (len(NETWORK.NEURONS))
constexpr int SH_NS = SH_LMAX + 2;     // smooth_net's Linear layers at most
constexpr int SH_NLAY = 2 + SH_NS + 1; // k_fit_shell_wgrad's tables: t_encoder's two, smooth_net's, the phase
constexpr int SH_NX_MAX = CORE_NX_MAX;

struct FitShellArgs {
  EqDev eq;             // the OU problem behind g0
  double T;
  const float* coeff;   // timestep_coeff (64)
  const float* phase;   // timestep_phase (64)
  const float* Wt[2];   // t_encoder: (64, 128), (64, 64)
  const float* bt[2];
  const float* Ws[SH_NS];  // smooth_net, layer k = 0 .. L + 1: (64, 128), L x (64, 64), (nx, 64)
  const float* bs[SH_NS];
  int L, nx, B, tiles, grad;
  int nt, ne;           // SH_NT and SH_NE as run-time values: fit_mv / fit_mvT keep their rolled loops
  const float* tx;      // (B, txstride): t | x
  int txstride;
  float* tau;           // (B, 64)
  float* s;             // (B)
  float* res;           // (B)
  float* res_x;         // (B, nx), grad only
  const float* dtau;    // (B, 64)
  const float* sbar;    // (B)
  float* ws;
  // float offsets into ws of the [unit][row] arrays; their row count is 64 (tiles + 1), the zero point is row
  // 64 tiles
  size_t offE;            // the embedding, 128 units
  size_t offAt, offPt;    // t_encoder's hidden layer: a and act'
  size_t offZt[2];        // zbar of t_encoder's two layers
  size_t offAs[SH_NS], offPs[SH_NS], offZs[SH_NS];  // smooth_net's ELU layers k = 0 .. L
  size_t offZL;           // the seed of smooth_net's output unit 0, one unit
  size_t offDW;           // the cotangent of omega, 64 units
};

__device__ __forceinline__ float shell_wave_sumf(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// smooth_net's output unit 0 at the zero point (lambda = 0, omega = phase) for the whole workgroup: a wave owns the
// units fit_mv gives it, its lanes run over the inputs.  Every workgroup gets the same bits.
__device__ __forceinline__ float shell_zero_out(const FitShellArgs& a, float (*zv)[SH_NE], int tid, int wv, int lane) {
  if (tid < SH_NT) {
    const double om = (double)a.phase[tid];
    zv[0][tid] = (float)sin(om);
    zv[0][SH_NT + tid] = (float)cos(om);
  }
  __syncthreads();
  int cur = 0;
  for (int k = 0; k <= a.L; ++k) {
    const int nin = k == 0 ? SH_NE : SH_NT;
    for (int jj = 0; jj < FIT_JB; ++jj) {
      const int j = wv * FIT_JB + jj;
      const float* w = a.Ws[k] + (size_t)j * nin;
      float p = w[lane] * zv[cur][lane];
      if (nin > SH_NT) p = fmaf(w[SH_NT + lane], zv[cur][SH_NT + lane], p);
      p = shell_wave_sumf(p);
      float v, d;
      fit_act<DPI_ACT_ELU>(p + a.bs[k][j], v, d);
      if (lane == 0) zv[cur ^ 1][j] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
  return shell_wave_sumf(a.Ws[a.L + 1][lane] * zv[cur][lane]) + a.bs[a.L + 1][0];
}

__global__ __launch_bounds__(FIT_NTH) void k_fit_shell_fwd(const FitShellArgs a) {
  __shared__ float bufE[SH_NE * FIT_ROWS];
  __shared__ float bufA[2][SH_NT * FIT_ROWS];
  __shared__ float zv[2][SH_NE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const bool zero = tile == a.tiles;  // the zero point's workgroup: every lane is the row lambda = 0
  const int row = tile * FIT_ROWS + lane;
  const bool live = !zero && row < a.B;
  const size_t R = (size_t)(a.tiles + 1) * FIT_ROWS;
  const int L = a.L;
  float* ws = a.ws;

  // emb = (sin omega, cos omega), omega = coeff lambda + phase in fp64 (omega reaches 100); a dead row has t = 0
  {
    const double lam = zero ? 0.0 : a.T - (live ? (double)a.tx[(size_t)row * a.txstride] : 0.0);
    float* E = ws + a.offE;
#pragma unroll 1
    for (int jj = 0; jj < FIT_JB; ++jj) {
      const int j = wv * FIT_JB + jj;
      const double om = fma((double)a.coeff[j], lam, (double)a.phase[j]);
      const float sn = (float)sin(om), cs = (float)cos(om);
      bufE[j * FIT_ROWS + lane] = sn;
      bufE[(SH_NT + j) * FIT_ROWS + lane] = cs;
      E[(size_t)j * R + row] = sn;
      E[(size_t)(SH_NT + j) * R + row] = cs;
    }
  }
  const float out0 = shell_zero_out(a, zv, tid, wv, lane);  // its first barrier also closes bufE

  // tau = t_encoder(emb)
  if (!zero) {
    const float* b0 = a.bt[0];
    const float* b1 = a.bt[1];
    float* A = ws + a.offAt;
    float* P = ws + a.offPt;
    fit_mv(a.Wt[0], a.nt, a.ne, bufE, wv, lane, [&](int j, float z) {
      float v, d;
      fit_act<DPI_ACT_ELU>(z + b0[j], v, d);
      bufA[0][j * FIT_ROWS + lane] = v;
      A[(size_t)j * R + row] = v;
      P[(size_t)j * R + row] = d;
    });
    __syncthreads();
    fit_mv(a.Wt[1], a.nt, a.nt, bufA[0], wv, lane, [&](int j, float z) {
      if (live) a.tau[(size_t)row * SH_NT + j] = z + b1[j];
    });
  }

  // s = smooth_net(emb)[0] - smooth_net(emb(0))[0]
  int cur = 1;
  for (int k = 0; k <= L; ++k) {
    const float* bk = a.bs[k];
    float* A = ws + a.offAs[k];
    float* P = ws + a.offPs[k];
    float* out = k == 0 ? bufA[1] : bufA[cur ^ 1];
    fit_mv(a.Ws[k], a.nt, k == 0 ? a.ne : a.nt, k == 0 ? bufE : bufA[cur], wv, lane, [&](int j, float z) {
      float v, d;
      fit_act<DPI_ACT_ELU>(z + bk[j], v, d);
      out[j * FIT_ROWS + lane] = v;
      A[(size_t)j * R + row] = v;
      P[(size_t)j * R + row] = d;
    });
    __syncthreads();
    if (k > 0) cur ^= 1;
  }
  if (zero) return;
  if (wv == 0) {
    const float* Wl = a.Ws[L + 1];
    float up[FIT_PS] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < SH_NT; ++j) up[j & (FIT_PS - 1)] = fmaf(Wl[j], bufA[cur][j * FIT_ROWS + lane], up[j & (FIT_PS - 1)]);
    const float o = ((up[0] + up[1]) + (up[2] + up[3])) + a.bs[L + 1][0];
    if (live) a.s[row] = o - out0;
  }

  // res = g(c x), res_x = c g_x(c x), c = exp(-lambda / 2): a wave per row, its lanes over the dimensions
  const EqDev& eq = a.eq;
  const int nx = a.nx;
  for (int rr = wv; rr < FIT_ROWS; rr += FIT_NW) {
    const int gr = tile * FIT_ROWS + rr;
    if (gr >= a.B) break;
    const float* xr = a.tx + (size_t)gr * a.txstride + 1;
    const double c = exp(-0.5 * (a.T - (double)xr[-1]));
    double st[NSG];
#pragma unroll
    for (int k = 0; k < NSG; ++k) st[k] = 0.0;
    for (int d = lane; d < nx; d += 64) Eq<DPI_EQ_OU>::gstat_d(eq, d, (float)(c * (double)xr[d]), st);
#pragma unroll
    for (int k = 0; k < NSG; ++k)
      if (k < eq.ncomp) st[k] = fit_wave_sum(st[k]);
    float rc[NSG];
    const float g = Eq<DPI_EQ_OU>::gfin_w(eq, st, rc);
    if (lane == 0) a.res[gr] = g;
    if (a.grad) {
      for (int d = lane; d < nx; d += 64) {
        const double X = (double)(float)(c * (double)xr[d]);
        double gx = 0.0;
#pragma unroll
        for (int k = 0; k < NSG; ++k)
          if (k < eq.ncomp) gx = fma((double)rc[k] * (X - (double)eq.mean[k * nx + d]), (double)eq.ivar[k * nx + d], gx);
        a.res_x[(size_t)gr * nx + d] = (float)(c * gx);
      }
    }
  }
}

struct FitShellLossArgs {
  const float *sp, *q, *s, *res, *res_x, *tx, *y;
  int txstride, ystride;
  int nx, B, tiles;
  int grad;     // 1: value + gradient losses, 0: the value loss alone
  int clipped;
  float beta, clip, kappa;
  float* losses;  // (2 + nx): total, v_loss, g_loss[nx]
  float* e;       // (B)
  float* r;       // (B, nx), grad only
  float* sbar;    // (B)
  double* part;   // (tiles, 1 + nx): a tile's sums of w rho, column 0 the value loss
};

__global__ __launch_bounds__(256) void k_fit_shell_loss(const FitShellLossArgs a) {
  __shared__ double sm[4][1 + SH_NX_MAX];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const int nx = a.nx;
  const double clip = (double)a.clip, invB = 1.0 / (double)a.B;
  double accv = 0.0, acc[2] = {0.0, 0.0};  // this wave's rows in order: the value column, columns lane and 64 + lane
  for (int rr = wv; rr < FIT_ROWS; rr += 4) {
    const int row = tile * FIT_ROWS + rr;
    if (row >= a.B) break;
    const double w = exp((double)a.beta * (double)a.tx[(size_t)row * a.txstride]);
    const double s = (double)a.s[row], sp = (double)a.sp[row], res = (double)a.res[row];
    const float* yr = a.y + (size_t)row * a.ystride;
    double rho, drho;
    fit_rho(s * sp + (1.0 - s) * res - (double)yr[0], a.clipped, clip, rho, drho);
    const double av = w * drho * invB;
    accv += w * rho;
    double sb = av * (sp - res);
    if (a.grad) {
      double sbp = 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int d = lane + 64 * h;
        if (d < nx) {
          const double q = (double)a.q[(size_t)row * nx + d], rx = (double)a.res_x[(size_t)row * nx + d];
          fit_rho(s * q + (1.0 - s) * rx - (double)yr[1 + d], a.clipped, clip, rho, drho);
          const double b = (double)a.kappa * w * drho * invB;
          a.r[(size_t)row * nx + d] = (float)(s * b);
          sbp += b * (q - rx);
          acc[h] += w * rho;
        }
      }
      sb += fit_wave_sum(sbp);
    }
    if (lane == 0) {
      a.e[row] = (float)(s * av);
      a.sbar[row] = (float)sb;
    }
  }
  if (lane == 0) sm[wv][0] = accv;
  sm[wv][1 + lane] = acc[0];
  sm[wv][1 + 64 + lane] = acc[1];
  __syncthreads();
  const int nc = a.grad ? 1 + nx : 1;
  for (int c = tid; c < nc; c += 256)
    a.part[(size_t)tile * (1 + nx) + c] = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
}

__global__ __launch_bounds__(256) void k_fit_shell_loss_sum(const FitShellLossArgs a) {
  __shared__ double sl[1 + SH_NX_MAX];
  const int tid = threadIdx.x;
  const int n0 = 1 + a.nx;
  const int nd = a.grad ? n0 : 1;
  for (int d = tid; d < n0; d += 256) {
    double s = 0.0;
    if (d < nd)
      for (int t = 0; t < a.tiles; ++t) s += a.part[(size_t)t * n0 + d];
    s /= (double)a.B;
    sl[d] = s;
    a.losses[1 + d] = (float)s;
  }
  __syncthreads();
  if (tid == 0) {
    double g = 0.0;
    for (int d = 1; d < nd; ++d) g += sl[d];
    a.losses[0] = (float)(a.grad ? sl[0] + (double)a.kappa * g : sl[0]);
  }
}

__global__ __launch_bounds__(FIT_NTH) void k_fit_shell_bwd(const FitShellArgs a) {
  __shared__ float bufE[SH_NE * FIT_ROWS];  // the cotangent of emb, both networks'
  __shared__ float bufA[2][SH_NT * FIT_ROWS];
  __shared__ double red[FIT_NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const bool zero = tile == a.tiles;
  const int row = tile * FIT_ROWS + lane;
  const bool live = !zero && row < a.B;
  const size_t R = (size_t)(a.tiles + 1) * FIT_ROWS;
  const int L = a.L;
  float* ws = a.ws;

  // the cotangent of smooth_net's output unit 0: sbar of the row; at the zero point -sum_rows sbar, rows in order
  float seed = live ? a.sbar[row] : 0.f;
  if (zero) {
    double p = 0.0;
    for (int r = tid; r < a.B; r += FIT_NTH) p += (double)a.sbar[r];
    p = fit_wave_sum(p);
    if (lane == 0) red[wv] = p;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < FIT_NW; ++w) tot += red[w];
    seed = (float)-tot;
  }
  if (wv == 0) ws[a.offZL + row] = seed;

  if (!zero) {
    // t_encoder: zbar_2 = taubar, zbar_1 = (W_2^T zbar_2) act'(z_1), embbar = W_1^T zbar_1
    float* Z2 = ws + a.offZt[1];
    float* Z1 = ws + a.offZt[0];
    const float* P = ws + a.offPt;
    for (int jj = 0; jj < FIT_JB; ++jj) {
      const int j = wv * FIT_JB + jj;
      const float v = live ? a.dtau[(size_t)row * SH_NT + j] : 0.f;
      bufA[0][j * FIT_ROWS + lane] = v;
      Z2[(size_t)j * R + row] = v;
    }
    __syncthreads();
    fit_mvT(a.Wt[1], a.nt, a.nt, bufA[0], wv, lane, [&](int i, float ab) {
      const size_t o = (size_t)i * R + row;
      const float zb = ab * P[o];
      Z1[o] = zb;
      bufA[1][i * FIT_ROWS + lane] = zb;
    });
    __syncthreads();
    fit_mvT(a.Wt[0], a.nt, a.ne, bufA[1], wv, lane, [&](int i, float ab) { bufE[i * FIT_ROWS + lane] = ab; });
    __syncthreads();
  } else {
    fit_owned(a.ne, wv, [&](int i) { bufE[i * FIT_ROWS + lane] = 0.f; });
  }

  // smooth_net: zbar_L = seed W_{L+1}[0] act'(z_L), then down; the thread that wrote an element of embbar adds to it
  {
    const float* Wl = a.Ws[L + 1];
    const float* P = ws + a.offPs[L];
    float* Z = ws + a.offZs[L];
    fit_owned(a.nt, wv, [&](int j) {
      const size_t o = (size_t)j * R + row;
      const float zb = seed * Wl[j] * P[o];
      Z[o] = zb;
      bufA[0][j * FIT_ROWS + lane] = zb;
    });
  }
  __syncthreads();
  int cur = 0;
  for (int k = L; k >= 1; --k) {
    const float* P = ws + a.offPs[k - 1];
    float* Z = ws + a.offZs[k - 1];
    float* out = bufA[cur ^ 1];
    fit_mvT(a.Ws[k], a.nt, a.nt, bufA[cur], wv, lane, [&](int i, float ab) {
      const size_t o = (size_t)i * R + row;
      const float zb = ab * P[o];
      Z[o] = zb;
      out[i * FIT_ROWS + lane] = zb;
    });
    __syncthreads();
    cur ^= 1;
  }
  fit_mvT(a.Ws[0], a.nt, a.ne, bufA[cur], wv, lane, [&](int i, float ab) { bufE[i * FIT_ROWS + lane] += ab; });
  __syncthreads();
  // omegabar_j = embbar_sin,j cos omega_j - embbar_cos,j sin omega_j
  {
    const float* E = ws + a.offE;
    float* DW = ws + a.offDW;
    for (int jj = 0; jj < FIT_JB; ++jj) {
      const int j = wv * FIT_JB + jj;
      const float sn = E[(size_t)j * R + row], cs = E[(size_t)(SH_NT + j) * R + row];
      DW[(size_t)j * R + row] = bufE[j * FIT_ROWS + lane] * cs - bufE[(SH_NT + j) * FIT_ROWS + lane] * sn;
    }
  }
}

// One table of k_fit_shell_wgrad: dW (nout, nin) = sum_rows z a^T and db (nout) = sum_rows z over the parked
// [unit][row] arrays Z and A.
struct ShellLayer {
  const float* Z;  // nz units; NULL: z = 1 (the phase: d phase = sum_rows omegabar)
  const float* A;  // nin units
  float* dW;
  float* db;       // NULL: none
  int nout, nin;
  int nz;          // units of Z; rows of dW from nz on are exact zeros (smooth_net's last weight: row 0 alone)
  int zrow;        // 1: the zero point's row is added after the batch's
  int zero_bias;   // 1: db is exact zeros (smooth_net's last bias cancels between the two evaluations)
};
struct FitShellWgradArgs {
  ShellLayer lay[SH_NLAY];
  int blk0[SH_NLAY + 1];  // first workgroup of table l; [nlay] = their count
  int nlay;
  int B, tiles;
};

__global__ __launch_bounds__(256) void k_fit_shell_wgrad(const FitShellWgradArgs a) {
  __shared__ float sZ[FIT_WT][FIT_CS], sA[FIT_WT][FIT_CS];
  const int tid = threadIdx.x;
  const size_t R = (size_t)(a.tiles + 1) * FIT_ROWS;
  const int blk = blockIdx.x;
  int l = 0;
  while (blk >= a.blk0[l + 1]) ++l;  // blk0[l] <= blk < blk0[l + 1]
  const ShellLayer& y = a.lay[l];
  const int nout = y.nout, nin = y.nin, nz = y.nz;
  const int nit = (nin + FIT_WT - 1) / FIT_WT;
  const int rel = blk - a.blk0[l];
  const int j0 = rel / nit * FIT_WT, i0 = (rel - rel / nit * nit) * FIT_WT;
  const float* Z = y.Z;
  const float* A = y.A;
  const int tj = tid >> 4, ti = tid & 15;
  const int j = j0 + tj, i = i0 + ti;
  const bool bias = i0 == 0 && ti == 0 && y.db != nullptr;
  double tot = 0.0, btot = 0.0;
  if (j0 < nz) {
    for (int r0 = 0; r0 < a.B; r0 += FIT_ROWS) {
      const int nr = min(FIT_ROWS, a.B - r0);
      __syncthreads();
      for (int k = tid; k < FIT_WT * FIT_ROWS; k += 256) {
        const int u = k >> 6, r = k & 63;
        if (r < nr) {
          const int ju = min(j0 + u, nz - 1), iu = min(i0 + u, nin - 1);
          const size_t row = (size_t)r0 + r;
          sZ[u][r] = Z ? Z[(size_t)ju * R + row] : 1.0f;
          sA[u][r] = A[(size_t)iu * R + row];
        }
      }
      __syncthreads();
      float c0 = 0.f, c1 = 0.f;
      double bc0 = 0.0, bc1 = 0.0;
      int r = 0;
      for (; r + 2 <= nr; r += 2) {
        c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
        c1 = fmaf(sZ[tj][r + 1], sA[ti][r + 1], c1);
        if (bias) {
          bc0 += (double)sZ[tj][r];
          bc1 += (double)sZ[tj][r + 1];
        }
      }
      if (r < nr) {
        c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
        if (bias) bc0 += (double)sZ[tj][r];
      }
      tot += (double)(c0 + c1);
      btot += bc0 + bc1;
    }
    if (y.zrow) {
      const size_t zr = (size_t)a.tiles * FIT_ROWS;
      const float z = Z ? Z[(size_t)min(j, nz - 1) * R + zr] : 1.0f;
      tot += (double)(z * A[(size_t)min(i, nin - 1) * R + zr]);
      btot += (double)z;
    }
  }
  if (j < nout && i < nin) y.dW[(size_t)j * nin + i] = j < nz ? (float)tot : 0.f;
  if (bias && j < nout) y.db[j] = (y.zero_bias || j >= nz) ? 0.f : (float)btot;
}

}  // namespace dpi
