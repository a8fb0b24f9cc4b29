// The fit's loss and parameter gradients on the device: what fit.gradient_objective /
// fit.value_objective and torch's double backward compute per training batch, for construct_mlp value
// networks, as two launches.
//
//   k_fit_rows   one workgroup per tile of 64 batch rows (lane = row, a wave owns blocks of FIT_JB
//                units of the layer it computes).  Runs the forward pass, the adjoint pass (grad_x u),
//                the loss seeds, the tangent pass of the adjoint chain and the reverse pass with a
//                run-time layer loop.  The vector a layer consumes is in LDS as [unit][row]; the
//                weights are read in place from torch's (out, in) tensors with wave-uniform addresses.
//                Per-layer state (a_l, lambda_l / zeta_l / zbar_l, delta_l, lambdabar_l) is parked in
//                the workspace as [unit][row]: the thread that wrote an element is the one that reads
//                it back.  No sum over rows happens here except the 64-row loss partials of a tile.
//   k_fit_wgrad  one workgroup per 16 x 16 tile of a layer's weight gradient.  It walks the batch rows
//                in order (64-row chunks staged in LDS, a chunk sum added to the running total), so
//                dW and db are bitwise reproducible and never accumulated into.  One more workgroup
//                sums the tiles' loss partials in tile order and writes `losses`.
//   k_fit_wgrad_step  the same launch with the Adam / AdamW update of every parameter in its epilogue
//                (dpi_fit_step): with k_fit_rows one whole training step, in place.
//
// Rows of the last tile past B are dead: they load zeros, run like live rows, and their loss terms and
// seeds are selected to +0; k_fit_wgrad never reads them.
//
// For a PISGradNet only nn_module runs here, as a differentiable primitive between torch's time networks
// and torch's loss: k_fit_core_fwd, k_fit_core_bwd and k_fit_core_wgrad at the end of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/dpi.h"
#include "dpi_device.h"

namespace dpi {

constexpr int FIT_ROWS = 64;      // batch rows per k_fit_rows workgroup
constexpr int FIT_NTH = 1024;     // its threads: 16 waves
constexpr int FIT_NW = FIT_NTH / 64;
constexpr int FIT_JB = 4;         // units a wave computes at once
constexpr int FIT_PS = 4;         // partial sums of a dot product (k mod 4), added pairwise at its end
constexpr int FIT_LMAX = 8;       // hidden layers
constexpr int FIT_WMAX = 256;     // hidden width
constexpr int FIT_NIN_MAX = 257;  // 1 + nx
constexpr int FIT_LDSW = 260;     // units an LDS vector buffer holds
constexpr int FIT_WT = 16;        // k_fit_wgrad: the weight tile is FIT_WT x FIT_WT, 256 threads
constexpr int FIT_CS = FIT_ROWS + 1;  // LDS row stride of a staged 64-row chunk

struct FitArgs {
  const float* W[FIT_LMAX + 1];  // layer l = 1 .. L + 1 at [l - 1]: (n[l], n[l - 1]) row-major
  const float* b[FIT_LMAX + 1];
  float* dW[FIT_LMAX + 1];
  float* db[FIT_LMAX + 1];
  int n[FIT_LMAX + 2];  // n[0] = 1 + nx, n[1 .. L] hidden widths, n[L + 1] = 1
  int L;
  int B, tiles;         // rows, 64-row tiles; the workspace row count is 64 tiles
  const float* tx;      // (B, n[0])
  const float* y;       // (B, ystride): y0 | grad labels
  int ystride;
  int grad;             // 1: value + gradient losses, 0: the value loss alone
  int clipped;          // 1: LossFnLinearClip(clip), 0: square
  float beta, clip, c;
  float* ws;
  // float offsets into ws of the [unit][row] arrays, by layer
  size_t offA[FIT_LMAX + 2];   // a_l, l = 1 .. L
  size_t offP[FIT_LMAX + 2];   // act'(z_l), l = 1 .. L
  size_t offD[FIT_LMAX + 2];   // delta_l, l = 1 .. L + 1 (delta_{L+1} = 1 on live rows)
  size_t offZ[FIT_LMAX + 2];   // lambda_l, then zeta_l, then zbar_l, l = 1 .. L + 1 (zbar_{L+1} = e)
  size_t offLB[FIT_LMAX + 2];  // lambdabar_l, l = 0 .. L
  size_t offPart;              // (tiles, n[0] + 1) partial sums of a tile, doubles (an even offset): column 0
                               // the value loss, 1 + d dimension d, n[0] the seeds e (db of the output layer)
  float* losses;               // (2 + nx): total, v_loss, g_loss[nx]
  int blk0[FIT_LMAX + 2];      // k_fit_wgrad: first workgroup of layer l at [l - 1]; [L + 1] = their count
};

// rho and rho' of the residual: the square, or LossFnLinearClip (x^2 inside |x| < clip, linear outside)
// The residuals, the loss terms and the seeds are formed in fp64 from the fp32 u and grad_x u and rounded
// once: u - y cancels, and a seed sum such as db of the output layer cancels again.
__device__ __forceinline__ void fit_rho(double x, int clipped, double clip, double& r, double& dr) {
  const double ax = fabs(x);
  if (clipped && !(ax < clip)) {
    r = 2.0 * clip * ax - clip * clip;
    dr = x > 0.0 ? 2.0 * clip : (x < 0.0 ? -2.0 * clip : 0.0);
  } else {
    r = x * x;
    dr = 2.0 * x;
  }
}

// phi(z) and phi'(z) to fp32 rounding (expm1f / expf / tanhf, as torch.nn.ELU / Tanh and their backward
// compute them): the label kernels' Act<>::f has an absolute error near z = 0, and its ELU derivative a + 1
// one at the size of 1, that a parameter gradient, unlike a Monte-Carlo label, shows.
template <int ACT>
__device__ __forceinline__ void fit_act(float z, float& v, float& d) {
  if (ACT == DPI_ACT_TANH) {
    v = tanhf(z);
    d = fmaf(-v, v, 1.0f);
  } else {
    v = z > 0.f ? z : expm1f(z);
    d = z > 0.f ? 1.0f : expf(z);  // not a + 1: that rounds at the size of 1 where phi' is small
  }
}
// phi'' from a = phi(z) and d = phi'(z)
template <int ACT>
__device__ __forceinline__ float fit_act_d2(float v, float d) {
  if (ACT == DPI_ACT_TANH) return -2.0f * v * d;
  return v > 0.f ? 0.f : d;
}
__device__ __forceinline__ double fit_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[j] = sum_i W[j][i] in[i], j over this wave's unit blocks; W is (nout, nin)
template <class Epi>
__device__ __forceinline__ void fit_mv(const float* __restrict__ W, int nout, int nin, const float* in, int wv,
                                       int lane, Epi&& epi) {
  for (int j0 = wv * FIT_JB; j0 < nout; j0 += FIT_NW * FIT_JB) {
    float acc[FIT_JB][FIT_PS];
    const float* wr[FIT_JB];
#pragma unroll
    for (int jj = 0; jj < FIT_JB; ++jj) {
#pragma unroll
      for (int p = 0; p < FIT_PS; ++p) acc[jj][p] = 0.f;
      wr[jj] = W + (size_t)min(j0 + jj, nout - 1) * nin;  // a row past the end repeats the last one, unused
    }
    int i = 0;
    for (; i + FIT_PS <= nin; i += FIT_PS) {
#pragma unroll
      for (int p = 0; p < FIT_PS; ++p) {
        const float x = in[(i + p) * FIT_ROWS + lane];
#pragma unroll
        for (int jj = 0; jj < FIT_JB; ++jj) acc[jj][p] = fmaf(wr[jj][i + p], x, acc[jj][p]);
      }
    }
    for (; i < nin; ++i) {
      const float x = in[i * FIT_ROWS + lane];
#pragma unroll
      for (int jj = 0; jj < FIT_JB; ++jj) acc[jj][0] = fmaf(wr[jj][i], x, acc[jj][0]);
    }
#pragma unroll
    for (int jj = 0; jj < FIT_JB; ++jj)
      if (j0 + jj < nout) epi(j0 + jj, (acc[jj][0] + acc[jj][1]) + (acc[jj][2] + acc[jj][3]));
  }
}

// out[i] = sum_j W[j][i] in[j], i over this wave's unit blocks; W is (nout, nin)
template <class Epi>
__device__ __forceinline__ void fit_mvT(const float* __restrict__ W, int nout, int nin, const float* in, int wv,
                                        int lane, Epi&& epi) {
  for (int i0 = wv * FIT_JB; i0 < nin; i0 += FIT_NW * FIT_JB) {
    float acc[FIT_JB][FIT_PS];
    int ic[FIT_JB];
#pragma unroll
    for (int ii = 0; ii < FIT_JB; ++ii) {
#pragma unroll
      for (int p = 0; p < FIT_PS; ++p) acc[ii][p] = 0.f;
      ic[ii] = min(i0 + ii, nin - 1);
    }
    int j = 0;
    for (; j + FIT_PS <= nout; j += FIT_PS) {
#pragma unroll
      for (int p = 0; p < FIT_PS; ++p) {
        const float x = in[(j + p) * FIT_ROWS + lane];
        const float* wr = W + (size_t)(j + p) * nin;
#pragma unroll
        for (int ii = 0; ii < FIT_JB; ++ii) acc[ii][p] = fmaf(wr[ic[ii]], x, acc[ii][p]);
      }
    }
    for (; j < nout; ++j) {
      const float x = in[j * FIT_ROWS + lane];
      const float* wr = W + (size_t)j * nin;
#pragma unroll
      for (int ii = 0; ii < FIT_JB; ++ii) acc[ii][0] = fmaf(wr[ic[ii]], x, acc[ii][0]);
    }
#pragma unroll
    for (int ii = 0; ii < FIT_JB; ++ii)
      if (i0 + ii < nin) epi(i0 + ii, (acc[ii][0] + acc[ii][1]) + (acc[ii][2] + acc[ii][3]));
  }
}

// the units of a width-n vector this wave owns (the blocks fit_mv / fit_mvT hand to their epilogues)
template <class F>
__device__ __forceinline__ void fit_owned(int n, int wv, F&& f) {
  for (int j0 = wv * FIT_JB; j0 < n; j0 += FIT_NW * FIT_JB)
    for (int jj = 0; jj < FIT_JB; ++jj)
      if (j0 + jj < n) f(j0 + jj);
}

template <int ACT>
__global__ __launch_bounds__(FIT_NTH) void k_fit_rows(const FitArgs a) {
  __shared__ float buf[2][FIT_LDSW * FIT_ROWS];
  __shared__ float e_s[FIT_ROWS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = blockIdx.x * FIT_ROWS + lane;
  const bool live = row < a.B;
  const size_t R = (size_t)a.tiles * FIT_ROWS;  // row count of the workspace arrays
  const int L = a.L;
  const int n0 = a.n[0];
  float* ws = a.ws;
  const double wgt = live ? exp((double)a.beta * (double)a.tx[(size_t)row * n0]) : 0.0;  // exp(beta t)
  // the tile's loss sums: fp64, so that the losses round once
  double* part = reinterpret_cast<double*>(ws + a.offPart) + (size_t)blockIdx.x * (n0 + 1);

  // a_0 = (t, x); dead rows are zeros
  for (int k = tid; k < FIT_ROWS * n0; k += FIT_NTH) {
    const int r = k / n0, i = k - r * n0;
    const int gr = blockIdx.x * FIT_ROWS + r;
    buf[0][i * FIT_ROWS + r] = gr < a.B ? a.tx[(size_t)gr * n0 + i] : 0.f;
  }
  __syncthreads();
  int cur = 0;

  // 1. forward
  for (int l = 1; l <= L; ++l) {
    const float* bl = a.b[l - 1];
    float* A = ws + a.offA[l];
    float* P = ws + a.offP[l];
    float* out = buf[cur ^ 1];
    fit_mv(a.W[l - 1], a.n[l], a.n[l - 1], buf[cur], wv, lane, [&](int j, float z) {
      float v, d;
      fit_act<ACT>(z + bl[j], v, d);
      out[j * FIT_ROWS + lane] = v;
      A[(size_t)j * R + row] = v;
      P[(size_t)j * R + row] = d;
    });
    __syncthreads();
    cur ^= 1;
  }
  const float* Wout = a.W[L];
  const int nL = a.n[L];
  // 3a. u, the value loss and its seed e = w rho'(u - y0) / B
  if (wv == 0) {
    float up[FIT_PS] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nL; ++j) up[j & (FIT_PS - 1)] = fmaf(Wout[j], buf[cur][j * FIT_ROWS + lane], up[j & (FIT_PS - 1)]);
    const float u = ((up[0] + up[1]) + (up[2] + up[3])) + a.b[L][0];
    const float y0 = live ? a.y[(size_t)row * a.ystride] : 0.f;
    double r, dr;
    fit_rho((double)u - (double)y0, a.clipped, (double)a.clip, r, dr);
    const double ed = live ? wgt * dr / (double)a.B : 0.0;
    const float e = (float)ed;
    e_s[lane] = e;
    ws[a.offZ[L + 1] + row] = e;
    ws[a.offD[L + 1] + row] = live ? 1.0f : 0.f;
    const double s = fit_wave_sum(live ? wgt * r : 0.0);
    const double se = fit_wave_sum(ed);
    if (lane == 0) {
      part[0] = s;
      part[n0] = se;
    }
  }
  __syncthreads();

  if (a.grad) {
    // 2. adjoint, downward: lambda_L = Wout^T, delta_l = lambda_l act'(z_l), lambda_{l-1} = W_l^T delta_l
    {
      float* P = ws + a.offP[L];
      float* Z = ws + a.offZ[L];
      float* D = ws + a.offD[L];
      fit_owned(nL, wv, [&](int j) {
        const size_t o = (size_t)j * R + row;
        const float lam = Wout[j];
        const float d = lam * P[o];
        Z[o] = lam;
        D[o] = d;
        buf[cur][j * FIT_ROWS + lane] = d;
      });
    }
    __syncthreads();
    for (int l = L; l >= 1; --l) {
      float* out = buf[cur ^ 1];
      if (l > 1) {
        float* P = ws + a.offP[l - 1];
        float* Z = ws + a.offZ[l - 1];
        float* D = ws + a.offD[l - 1];
        fit_mvT(a.W[l - 1], a.n[l], a.n[l - 1], buf[cur], wv, lane, [&](int i, float lam) {
          const size_t o = (size_t)i * R + row;
          const float d = lam * P[o];
          Z[o] = lam;
          D[o] = d;
          out[i * FIT_ROWS + lane] = d;
        });
      } else {
        // lambda_0: columns 1 .. nx are grad_x u.  3b. the gradient losses and the seeds
        // r_d = c w rho'(d_d u - y_d) / B = lambdabar_0 (its t column is 0)
        float* LB = ws + a.offLB[0];
        fit_mvT(a.W[0], a.n[1], n0, buf[cur], wv, lane, [&](int i, float lam) {
          float lb = 0.f;
          if (i > 0) {
            const float yd = live ? a.y[(size_t)row * a.ystride + i] : 0.f;
            double r, dr;
            fit_rho((double)lam - (double)yd, a.clipped, (double)a.clip, r, dr);
            lb = live ? (float)((double)a.c * wgt * dr / (double)a.B) : 0.f;
            const double s = fit_wave_sum(live ? wgt * r : 0.0);
            if (lane == 0) part[i] = s;
          }
          LB[(size_t)i * R + row] = lb;
          out[i * FIT_ROWS + lane] = lb;
        });
      }
      __syncthreads();
      cur ^= 1;
    }
    // 4. tangent of the adjoint chain, upward: deltabar_l = W_l lambdabar_{l-1},
    // lambdabar_l = deltabar_l act'(z_l), zeta_l = deltabar_l lambda_l act''(z_l)
    for (int l = 1; l <= L; ++l) {
      float* A = ws + a.offA[l];
      float* P = ws + a.offP[l];
      float* Z = ws + a.offZ[l];
      float* LB = ws + a.offLB[l];
      float* out = buf[cur ^ 1];
      fit_mv(a.W[l - 1], a.n[l], a.n[l - 1], buf[cur], wv, lane, [&](int j, float db) {
        const size_t o = (size_t)j * R + row;
        const float d = P[o];
        const float lb = db * d;
        LB[o] = lb;
        out[j * FIT_ROWS + lane] = lb;
        Z[o] = db * Z[o] * fit_act_d2<ACT>(A[o], d);
      });
      __syncthreads();
      cur ^= 1;
    }
  }

  // 5. reverse, downward: abar_L = e Wout^T, zbar_l = abar_l act'(z_l) + zeta_l, abar_{l-1} = W_l^T zbar_l
  {
    float* P = ws + a.offP[L];
    float* Z = ws + a.offZ[L];
    const float e = e_s[lane];
    fit_owned(nL, wv, [&](int j) {
      const size_t o = (size_t)j * R + row;
      float zb = e * Wout[j] * P[o];
      if (a.grad) zb += Z[o];
      Z[o] = zb;
      buf[cur][j * FIT_ROWS + lane] = zb;
    });
  }
  __syncthreads();
  for (int l = L; l >= 2; --l) {
    float* P = ws + a.offP[l - 1];
    float* Z = ws + a.offZ[l - 1];
    float* out = buf[cur ^ 1];
    fit_mvT(a.W[l - 1], a.n[l], a.n[l - 1], buf[cur], wv, lane, [&](int i, float ab) {
      const size_t o = (size_t)i * R + row;
      float zb = ab * P[o];
      if (a.grad) zb += Z[o];
      Z[o] = zb;
      out[i * FIT_ROWS + lane] = zb;
    });
    __syncthreads();
    cur ^= 1;
  }
}

// What k_fit_wgrad_step takes beside FitArgs: the Adam state of every parameter (the tables of FitArgs' W
// and b, which this launch writes) and the step's scalars, each formed on the host in double and rounded
// once, as torch rounds the Python scalars of its update.
struct FitAdam {
  float* mW[FIT_LMAX + 1];  // exp_avg of W_l and b_l at [l - 1]
  float* mb[FIT_LMAX + 1];
  float* vW[FIT_LMAX + 1];  // exp_avg_sq
  float* vb[FIT_LMAX + 1];
  float omb1, beta2, omb2, eps, wd;  // 1 - beta1, beta2, 1 - beta2
  float decay;                       // 1 - lr wd
  float step_size, bc2_sqrt;         // lr / (1 - beta1^step), sqrt(1 - beta2^step)
  int decoupled;                     // 1: AdamW (w *= decay), 0: Adam with L2 weight decay (g += wd w)
};
struct FitStepArgs {
  FitArgs f;  // dW / db entries may be NULL: the gradient is not stored
  FitAdam o;
};

// One parameter's update from its gradient, fp32, in the order of torch's single-tensor Adam.  No two of
// the operations are contracted into an fma: each rounds on its own, as torch's separate kernels round.
__device__ __forceinline__ void fit_adam(const FitAdam& o, float g, float* __restrict__ w, float* __restrict__ m,
                                         float* __restrict__ v) {
#pragma clang fp contract(off)
  float wv = *w, mv = *m, vv = *v;
  if (o.wd != 0.f) {
    if (o.decoupled)
      wv *= o.decay;
    else
      g += o.wd * wv;
  }
  mv += (g - mv) * o.omb1;
  vv = o.beta2 * vv + o.omb2 * g * g;
  wv -= o.step_size * (mv / (sqrtf(vv) / o.bc2_sqrt + o.eps));
  *w = wv;
  *m = mv;
  *v = vv;
}

// dW_l = sum_rows delta_l lambdabar_{l-1}^T + zbar_l a_{l-1}^T, db_l = sum_rows zbar_l, rows in order.
// STEP: the thread that holds the final total of a gradient element also applies the Adam update of its
// parameter (o, else unused); nothing in this launch reads the weights, k_fit_rows before it is their only
// reader.
template <bool STEP>
__device__ __forceinline__ void fit_wgrad(const FitArgs& a, const FitAdam* o) {
  __shared__ float sD[FIT_WT][FIT_CS], sZ[FIT_WT][FIT_CS], sLB[FIT_WT][FIT_CS], sA[FIT_WT][FIT_CS];
  __shared__ double sl[FIT_LDSW];
  const int tid = threadIdx.x;
  const int L = a.L;
  const int n0 = a.n[0];
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int blk = blockIdx.x;
  if (blk == a.blk0[L + 1]) {
    // the losses: tile partials in tile order, then the dimensions in order
    const int nd = a.grad ? n0 : 1;
    const double* part = reinterpret_cast<const double*>(a.ws + a.offPart);
    for (int d = tid; d < n0; d += 256) {
      double s = 0.0;
      if (d < nd)
        for (int t = 0; t < a.tiles; ++t) s += part[(size_t)t * (n0 + 1) + d];
      s /= (double)a.B;
      sl[d] = s;
      a.losses[1 + d] = (float)s;
    }
    __syncthreads();
    if (tid == 1) {  // db of the output layer: the sum of the seeds e
      double se = 0.0;
      for (int t = 0; t < a.tiles; ++t) se += part[(size_t)t * (n0 + 1) + n0];
      if (!STEP || a.db[L]) a.db[L][0] = (float)se;
      if (STEP) fit_adam(*o, (float)se, const_cast<float*>(a.b[L]), o->mb[L], o->vb[L]);
    }
    if (tid == 0) {
      double g = 0.0;
      for (int d = 1; d < nd; ++d) g += sl[d];
      a.losses[0] = (float)(a.grad ? sl[0] + (double)a.c * g : sl[0]);
    }
    return;
  }
  int l = 1;
  while (blk >= a.blk0[l]) ++l;  // blk0[l - 1] <= blk < blk0[l]
  const int nout = a.n[l], nin = a.n[l - 1];
  const int nit = (nin + FIT_WT - 1) / FIT_WT;
  const int rel = blk - a.blk0[l - 1];
  const int j0 = rel / nit * FIT_WT, i0 = (rel - rel / nit * nit) * FIT_WT;
  const float* D = a.ws + a.offD[l];
  const float* Z = a.ws + a.offZ[l];
  const float* LB = a.ws + a.offLB[l - 1];
  const float* A = a.ws + a.offA[l - 1];  // l = 1: tx itself
  const int tj = tid >> 4, ti = tid & 15;
  const bool bias = i0 == 0 && ti == 0 && l <= L;  // db of the output layer comes with the losses
  double tot = 0.0, btot = 0.0;  // the running totals over the chunks, and the bias sums throughout, in fp64
  for (int r0 = 0; r0 < a.B; r0 += FIT_ROWS) {
    const int nr = min(FIT_ROWS, a.B - r0);
    __syncthreads();
    for (int k = tid; k < FIT_WT * FIT_ROWS; k += 256) {
      const int u = k >> 6, r = k & 63;
      if (r < nr) {
        const int j = min(j0 + u, nout - 1), i = min(i0 + u, nin - 1);
        const size_t row = (size_t)r0 + r;
        sZ[u][r] = Z[(size_t)j * R + row];
        sA[u][r] = l == 1 ? a.tx[row * n0 + i] : A[(size_t)i * R + row];
        if (a.grad) {
          sD[u][r] = D[(size_t)j * R + row];
          sLB[u][r] = LB[(size_t)i * R + row];
        }
      }
    }
    __syncthreads();
    // the chunk's sum: the two products and the even / odd rows apart, added pairwise
    float c0 = 0.f, c1 = 0.f, g0 = 0.f, g1 = 0.f;
    double bc0 = 0.0, bc1 = 0.0;
    int r = 0;
    for (; r + 2 <= nr; r += 2) {
      c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
      c1 = fmaf(sZ[tj][r + 1], sA[ti][r + 1], c1);
      if (a.grad) {
        g0 = fmaf(sD[tj][r], sLB[ti][r], g0);
        g1 = fmaf(sD[tj][r + 1], sLB[ti][r + 1], g1);
      }
      if (bias) {
        bc0 += (double)sZ[tj][r];
        bc1 += (double)sZ[tj][r + 1];
      }
    }
    if (r < nr) {
      c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
      if (a.grad) g0 = fmaf(sD[tj][r], sLB[ti][r], g0);
      if (bias) bc0 += (double)sZ[tj][r];
    }
    tot += (double)((c0 + c1) + (g0 + g1));
    btot += bc0 + bc1;
  }
  const int j = j0 + tj, i = i0 + ti;
  if (j < nout && i < nin) {
    const size_t e = (size_t)j * nin + i;
    if (!STEP || a.dW[l - 1]) a.dW[l - 1][e] = (float)tot;
    if (STEP) fit_adam(*o, (float)tot, const_cast<float*>(a.W[l - 1]) + e, o->mW[l - 1] + e, o->vW[l - 1] + e);
  }
  if (bias && j < nout) {
    if (!STEP || a.db[l - 1]) a.db[l - 1][j] = (float)btot;
    if (STEP) fit_adam(*o, (float)btot, const_cast<float*>(a.b[l - 1]) + j, o->mb[l - 1] + j, o->vb[l - 1] + j);
  }
}

__global__ __launch_bounds__(256) void k_fit_wgrad(const FitArgs a) { fit_wgrad<false>(a, nullptr); }
// the whole training step's second launch (dpi_fit_step)
__global__ __launch_bounds__(256) void k_fit_wgrad_step(const FitStepArgs a) { fit_wgrad<true>(a.f, &a.o); }

// ---- PISGradNet's nn_module as a differentiable primitive ("The PISGradNet core") ----
//
// Rows a_0 = (tau (64), x (nx)); N = nn_module(a_0) (nx outputs), sp = x . N, q = d sp / d x = N +
// (J^T x)[x columns].  The loss around (sp, q) is torch's; its cotangents e = d loss / d sp and
// r = d loss / d q come back to the second entry.  ELU only.
//
//   k_fit_core_fwd    passes 1 (forward) and 2 (adjoint with delta_{L+1} = x): writes sp, q and parks the state
//   k_fit_core_bwd    passes 3 (tangent from lambdabar_0 = (0, r)) and 4 (reverse from zbar_{L+1} = e x + r, down
//                     to abar_0, whose tau columns are the gradient of tau)
//   k_fit_core_wgrad  k_fit_wgrad's row walk for every layer, the nx-wide output layer included
//
// Same tile as k_fit_rows (64 rows, lane = row, fit_mv / fit_mvT), but widths run to 512, so there is one LDS
// vector, not two: a layer's result is parked first ([unit][row], as k_fit_rows parks it anyway) and, after
// a barrier, staged from the workgroup's own parked columns for the next layer.  a_0 is parked as well: its x
// columns are delta_{L+1} of the output layer's tangent term.
constexpr int CORE_LMAX = 4;     // hidden layers
constexpr int CORE_WMAX = 512;   // hidden width: CORE_WMAX x FIT_ROWS floats are the 128 KB LDS vector
constexpr int CORE_NT = 64;      // tau columns (PISGradNet.channels)
constexpr int CORE_NX_MAX = 128;

struct FitCoreArgs {
  const float* W[CORE_LMAX + 1];  // layer l = 1 .. L + 1 at [l - 1]: (n[l], n[l - 1]) row-major
  const float* b[CORE_LMAX + 1];
  float* dW[CORE_LMAX + 1];
  float* db[CORE_LMAX + 1];
  int n[CORE_LMAX + 2];  // n[0] = 64 + nx, n[1 .. L] hidden widths, n[L + 1] = nx
  int L;
  int B, tiles;
  int grad;              // forward: form q (pass 2); backward: r is given (pass 3)
  const float* tau;      // (B, taustride >= 64)
  const float* x;        // (B, xstride >= nx)
  int taustride, xstride;
  float* sp;             // (B)
  float* q;              // (B, nx)
  const float* e;        // (B)
  const float* r;        // (B, nx)
  float* dtau;           // (B, 64)
  float* ws;
  size_t offA[CORE_LMAX + 2];   // a_l, l = 0 .. L
  size_t offP[CORE_LMAX + 2];   // act'(z_l), l = 1 .. L
  size_t offD[CORE_LMAX + 2];   // delta_l, l = 1 .. L; [L + 1] is the x columns of a_0
  size_t offZ[CORE_LMAX + 2];   // lambda_l, then zeta_l, then zbar_l, l = 1 .. L; zbar_{L+1}
  size_t offLB[CORE_LMAX + 2];  // lambdabar_l, l = 0 .. L
  size_t offN;                  // N, nx units
  int blk0[CORE_LMAX + 2];      // k_fit_core_wgrad: first workgroup of layer l at [l - 1]; [L + 1] = their count
};

// the LDS vector <- the tile's columns of a parked [unit][row] array of n units
__device__ __forceinline__ void core_stage(float* buf, const float* __restrict__ src, int n, size_t R, int tile,
                                           int tid) {
  for (int k = tid; k < n * FIT_ROWS; k += FIT_NTH)
    buf[k] = src[(size_t)(k >> 6) * R + (size_t)tile * FIT_ROWS + (k & 63)];
}

__global__ __launch_bounds__(FIT_NTH) void k_fit_core_fwd(const FitCoreArgs a) {
  __shared__ float buf[CORE_WMAX * FIT_ROWS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const int row = tile * FIT_ROWS + lane;
  const bool live = row < a.B;
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int L = a.L;
  const int n0 = a.n[0], nx = a.n[L + 1];
  float* ws = a.ws;

  // a_0 = (tau, x), parked and staged; dead rows are zeros
  {
    float* A0 = ws + a.offA[0];
    for (int k = tid; k < FIT_ROWS * n0; k += FIT_NTH) {
      const int r = k / n0, i = k - r * n0;
      const int gr = tile * FIT_ROWS + r;
      float v = 0.f;
      if (gr < a.B)
        v = i < CORE_NT ? a.tau[(size_t)gr * a.taustride + i] : a.x[(size_t)gr * a.xstride + (i - CORE_NT)];
      buf[i * FIT_ROWS + r] = v;
      A0[(size_t)i * R + gr] = v;
    }
  }
  __syncthreads();

  // 1. forward
  for (int l = 1; l <= L; ++l) {
    const float* bl = a.b[l - 1];
    float* A = ws + a.offA[l];
    float* P = ws + a.offP[l];
    fit_mv(a.W[l - 1], a.n[l], a.n[l - 1], buf, wv, lane, [&](int j, float z) {
      float v, d;
      fit_act<DPI_ACT_ELU>(z + bl[j], v, d);
      A[(size_t)j * R + row] = v;
      P[(size_t)j * R + row] = d;
    });
    __syncthreads();
    core_stage(buf, A, a.n[l], R, tile, tid);
    __syncthreads();
  }
  // N = W_{L+1} a_L + b_{L+1}
  float* N = ws + a.offN;
  {
    const float* bo = a.b[L];
    fit_mv(a.W[L], nx, a.n[L], buf, wv, lane, [&](int j, float z) { N[(size_t)j * R + row] = z + bo[j]; });
  }
  __syncthreads();
  // delta_{L+1} = x; sp = x . N, units in order as 4 partial sums
  core_stage(buf, ws + a.offD[L + 1], nx, R, tile, tid);
  __syncthreads();
  if (wv == 0) {
    float s[FIT_PS] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nx; ++j)
      s[j & (FIT_PS - 1)] = fmaf(buf[j * FIT_ROWS + lane], N[(size_t)j * R + row], s[j & (FIT_PS - 1)]);
    if (live) a.sp[row] = (s[0] + s[1]) + (s[2] + s[3]);
  }
  if (!a.grad) return;

  // 2. adjoint, downward: lambda_L = W_{L+1}^T x, delta_l = lambda_l act'(z_l), lambda_{l-1} = W_l^T delta_l
  for (int l = L + 1; l >= 2; --l) {
    float* P = ws + a.offP[l - 1];
    float* Z = ws + a.offZ[l - 1];
    float* D = ws + a.offD[l - 1];
    fit_mvT(a.W[l - 1], a.n[l], a.n[l - 1], buf, wv, lane, [&](int i, float lam) {
      const size_t o = (size_t)i * R + row;
      Z[o] = lam;
      D[o] = lam * P[o];
    });
    __syncthreads();
    core_stage(buf, D, a.n[l - 1], R, tile, tid);
    __syncthreads();
  }
  // lambda_0: its x columns complete q = N + (J^T x)
  fit_mvT(a.W[0], a.n[1], n0, buf, wv, lane, [&](int i, float lam) {
    if (i >= CORE_NT && live) a.q[(size_t)row * nx + (i - CORE_NT)] = N[(size_t)(i - CORE_NT) * R + row] + lam;
  });
}

__global__ __launch_bounds__(FIT_NTH) void k_fit_core_bwd(const FitCoreArgs a) {
  __shared__ float buf[CORE_WMAX * FIT_ROWS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const int row = tile * FIT_ROWS + lane;
  const bool live = row < a.B;
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int L = a.L;
  const int n0 = a.n[0], nx = a.n[L + 1];
  float* ws = a.ws;

  if (a.grad) {
    // 3. tangent of the adjoint chain, upward, from lambdabar_0 = (0_tau, r)
    {
      float* LB0 = ws + a.offLB[0];
      for (int k = tid; k < FIT_ROWS * n0; k += FIT_NTH) {
        const int r = k / n0, i = k - r * n0;
        const int gr = tile * FIT_ROWS + r;
        const float v = (gr < a.B && i >= CORE_NT) ? a.r[(size_t)gr * nx + (i - CORE_NT)] : 0.f;
        buf[i * FIT_ROWS + r] = v;
        LB0[(size_t)i * R + gr] = v;
      }
    }
    __syncthreads();
    for (int l = 1; l <= L; ++l) {
      float* A = ws + a.offA[l];
      float* P = ws + a.offP[l];
      float* Z = ws + a.offZ[l];
      float* LB = ws + a.offLB[l];
      fit_mv(a.W[l - 1], a.n[l], a.n[l - 1], buf, wv, lane, [&](int j, float db) {
        const size_t o = (size_t)j * R + row;
        const float d = P[o];
        LB[o] = db * d;
        Z[o] = db * Z[o] * fit_act_d2<DPI_ACT_ELU>(A[o], d);
      });
      __syncthreads();
      if (l < L) {
        core_stage(buf, LB, a.n[l], R, tile, tid);
        __syncthreads();
      }
    }
  }

  // 4. reverse, downward: zbar_{L+1} = e x + r, zbar_l = abar_l act'(z_l) + zeta_l, abar_{l-1} = W_l^T zbar_l
  {
    float* ZO = ws + a.offZ[L + 1];
    const float* X = ws + a.offD[L + 1];
    for (int k = tid; k < FIT_ROWS * nx; k += FIT_NTH) {
      const int r = k / nx, i = k - r * nx;
      const int gr = tile * FIT_ROWS + r;
      float v = 0.f;
      if (gr < a.B) {
        v = a.e[gr] * X[(size_t)i * R + gr];
        if (a.grad) v += a.r[(size_t)gr * nx + i];
      }
      buf[i * FIT_ROWS + r] = v;
      ZO[(size_t)i * R + gr] = v;
    }
  }
  __syncthreads();
  for (int l = L + 1; l >= 2; --l) {
    float* P = ws + a.offP[l - 1];
    float* Z = ws + a.offZ[l - 1];
    fit_mvT(a.W[l - 1], a.n[l], a.n[l - 1], buf, wv, lane, [&](int i, float ab) {
      const size_t o = (size_t)i * R + row;
      float zb = ab * P[o];
      if (a.grad) zb += Z[o];
      Z[o] = zb;
    });
    __syncthreads();
    core_stage(buf, Z, a.n[l - 1], R, tile, tid);
    __syncthreads();
  }
  // abar_0: its tau columns
  fit_mvT(a.W[0], a.n[1], n0, buf, wv, lane, [&](int i, float ab) {
    if (i < CORE_NT && live) a.dtau[(size_t)row * CORE_NT + i] = ab;
  });
}

// dW_l = sum_rows delta_l lambdabar_{l-1}^T + zbar_l a_{l-1}^T, db_l = sum_rows zbar_l for l = 1 .. L + 1, rows in
// order (k_fit_wgrad's walk; here a_0 is parked and the output layer has nx units and a bias like the others)
__global__ __launch_bounds__(256) void k_fit_core_wgrad(const FitCoreArgs a) {
  __shared__ float sD[FIT_WT][FIT_CS], sZ[FIT_WT][FIT_CS], sLB[FIT_WT][FIT_CS], sA[FIT_WT][FIT_CS];
  const int tid = threadIdx.x;
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int blk = blockIdx.x;
  int l = 1;
  while (blk >= a.blk0[l]) ++l;  // blk0[l - 1] <= blk < blk0[l]
  const int nout = a.n[l], nin = a.n[l - 1];
  const int nit = (nin + FIT_WT - 1) / FIT_WT;
  const int rel = blk - a.blk0[l - 1];
  const int j0 = rel / nit * FIT_WT, i0 = (rel - rel / nit * nit) * FIT_WT;
  const float* D = a.ws + a.offD[l];
  const float* Z = a.ws + a.offZ[l];
  const float* LB = a.ws + a.offLB[l - 1];
  const float* A = a.ws + a.offA[l - 1];
  const int tj = tid >> 4, ti = tid & 15;
  const bool bias = i0 == 0 && ti == 0;
  double tot = 0.0, btot = 0.0;
  for (int r0 = 0; r0 < a.B; r0 += FIT_ROWS) {
    const int nr = min(FIT_ROWS, a.B - r0);
    __syncthreads();
    for (int k = tid; k < FIT_WT * FIT_ROWS; k += 256) {
      const int u = k >> 6, r = k & 63;
      if (r < nr) {
        const int j = min(j0 + u, nout - 1), i = min(i0 + u, nin - 1);
        const size_t row = (size_t)r0 + r;
        sZ[u][r] = Z[(size_t)j * R + row];
        sA[u][r] = A[(size_t)i * R + row];
        if (a.grad) {
          sD[u][r] = D[(size_t)j * R + row];
          sLB[u][r] = LB[(size_t)i * R + row];
        }
      }
    }
    __syncthreads();
    float c0 = 0.f, c1 = 0.f, g0 = 0.f, g1 = 0.f;
    double bc0 = 0.0, bc1 = 0.0;
    int r = 0;
    for (; r + 2 <= nr; r += 2) {
      c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
      c1 = fmaf(sZ[tj][r + 1], sA[ti][r + 1], c1);
      if (a.grad) {
        g0 = fmaf(sD[tj][r], sLB[ti][r], g0);
        g1 = fmaf(sD[tj][r + 1], sLB[ti][r + 1], g1);
      }
      if (bias) {
        bc0 += (double)sZ[tj][r];
        bc1 += (double)sZ[tj][r + 1];
      }
    }
    if (r < nr) {
      c0 = fmaf(sZ[tj][r], sA[ti][r], c0);
      if (a.grad) g0 = fmaf(sD[tj][r], sLB[ti][r], g0);
      if (bias) bc0 += (double)sZ[tj][r];
    }
    tot += (double)((c0 + c1) + (g0 + g1));
    btot += bc0 + bc1;
  }
  const int j = j0 + tj, i = i0 + ti;
  if (j < nout && i < nin) a.dW[l - 1][(size_t)j * nin + i] = (float)tot;
  if (bias && j < nout) a.db[l - 1][j] = (float)btot;
}

}  // namespace dpi
