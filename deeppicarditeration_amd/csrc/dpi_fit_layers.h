// The layer-wise form of the PISGradNet core (TRAIN.CORE_FORM: layers; DESIGN.md §5.1, "The layer-wise form").
//
// The same four passes, workspace arrays and weight-gradient launch as k_fit_core_fwd / k_fit_core_bwd
// (dpi_fit.h), but one launch per layer and pass, its grid over (64-row tile x block of 16 output units), so
// that a 512-wide layer at B = 512 is 8 x 32 = 256 workgroups and not 8.  Every product of a step has one of
// two shapes over the parked [unit][row] arrays,
//
//   LAY_N   OUT[u][row] = sum_k W[u][k] IN[k][row]   forward and tangent passes (fit_mv's job)
//   LAY_T   OUT[i][row] = sum_j W[j][i] IN[j][row]   adjoint and reverse passes (fit_mvT's job)
//
// and k_fit_layer<ORI, EPI> is both, with the epilogue of the pass.  A workgroup is 4 waves; wave w owns the
// 16 rows w of the tile and all 16 units, as one v_mfma_f32_16x16x4_f32 tile (units are M, rows are N): the
// result is a k-ordered fp32 fmaf chain, exact fp32 with no wider accumulation.  The k blocks of 4 go round
// four accumulators, added pairwise at the end as fit_mv adds its four partial sums, so the summation order
// is fixed and a result is bitwise reproducible.  The operands of LAY_KC k at a time are staged in LDS through
// registers, the next chunk's loads in flight under this chunk's products; what lies past a width is selected
// to 0 on load and never addressed, units past the width are never stored.
//
// Rows of the last tile past B are dead as in dpi_fit.h: k_fit_layers_a0 and k_fit_layers_seed park zeros
// for them, every launch computes and parks all 64 rows of a tile from what the launches before it parked,
// and only sp, q and dtau are masked.  No launch reads a workspace element that an earlier launch of the
// same forward / backward pair did not write.
#pragma once
#include "dpi_fit.h"

namespace dpi {

constexpr int LAY_UT = 16;                  // output units per workgroup: the MFMA's M
constexpr int LAY_NTH = 256;                // 4 waves, one 16-row fragment of the tile each
constexpr int LAY_KC = 128;                 // k staged at once
constexpr int LAY_IS = FIT_ROWS + 16;       // LDS row stride of the staged IN: the 4 k of a fragment on 4 bank groups
constexpr int LAY_WS = LAY_KC + 4;          // LDS unit stride of the staged W: 16 units x 4 k on 64 banks

enum { LAY_N = 0, LAY_T = 1 };
enum {
  LAY_ACT = 0,   // pass 1: a_l = phi(z + b), phi' parked                      (LAY_N, IN = a_{l-1})
  LAY_OUT = 1,   // pass 1: N = z + b                                          (LAY_N, IN = a_L)
  LAY_ADJ = 2,   // pass 2: lambda_{l-1}, delta_{l-1} = lambda phi'            (LAY_T, IN = delta_l)
  LAY_Q = 3,     // pass 2: q = N + lambda_0[x columns]                        (LAY_T, IN = delta_1, units >= 64)
  LAY_TAN = 4,   // pass 3: lambdabar_l = dbar phi', zeta_l = dbar lambda phi''  (LAY_N, IN = lambdabar_{l-1})
  LAY_REV = 5,   // pass 4: zbar_{l-1} = abar phi' (+ zeta)                    (LAY_T, IN = zbar_l)
  LAY_DTAU = 6   // pass 4: dtau = abar_0[tau columns]                         (LAY_T, IN = zbar_1, units < 64)
};

typedef float lay_f4 __attribute__((ext_vector_type(4)));

// Layer l = 1 .. L + 1 of `a` (W = a.W[l - 1], (n[l], n[l - 1]) row-major).  Grid (tiles, unit blocks).
template <int ORI, int EPI>
__global__ __launch_bounds__(LAY_NTH) void k_fit_layer(const FitCoreArgs a, const int l) {
  __shared__ float sIn[LAY_KC * LAY_IS];
  __shared__ float sW[LAY_UT * LAY_WS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int tile = blockIdx.x;
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int nrow = a.n[l], ncol = a.n[l - 1];
  const int K = ORI == LAY_N ? ncol : nrow;   // the summed index
  const int NU = ORI == LAY_N ? nrow : ncol;  // the output units
  const int u0 = ((int)blockIdx.y + (EPI == LAY_Q ? CORE_NT / LAY_UT : 0)) * LAY_UT;
  const float* __restrict__ W = a.W[l - 1];
  float* ws = a.ws;
  const float* IN = ws + (EPI == LAY_ACT || EPI == LAY_OUT ? a.offA[l - 1]
                          : EPI == LAY_TAN                 ? a.offLB[l - 1]
                          : EPI == LAY_ADJ || EPI == LAY_Q ? a.offD[l]
                                                           : a.offZ[l]) + (size_t)tile * FIT_ROWS;

  lay_f4 acc[FIT_PS];
#pragma unroll
  for (int p = 0; p < FIT_PS; ++p) acc[p] = lay_f4{0.f, 0.f, 0.f, 0.f};
  const int fu = lane & 15, fk = lane >> 4;  // this lane's unit (A) or row (B) of the fragment, and its k of 4

  // A chunk of LAY_KC k goes global -> registers -> LDS: the loads of the next chunk are issued before the
  // products of this one, all LAY_IN + LAY_WN of a thread in flight at once.  Element i of a thread is row
  // 4 i + wv of IN (column lane), and of W unit 2 i + (tid >> 7), k tid & 127 (LAY_N: k runs along a row of W)
  // or k 16 i + (tid >> 4), unit tid & 15 (LAY_T: units run along a row of W).
  constexpr int LAY_IN = LAY_KC * FIT_ROWS / LAY_NTH, LAY_WN = LAY_UT * LAY_KC / LAY_NTH;
  float vi[LAY_IN], vw[LAY_WN];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < LAY_IN; ++i) {
      const int k = k0 + 4 * i + wv;
      vi[i] = 0.f;
      if (k < K) vi[i] = IN[(size_t)k * R + lane];
    }
#pragma unroll
    for (int i = 0; i < LAY_WN; ++i) {
      const int u = u0 + (ORI == LAY_N ? 2 * i + (tid >> 7) : (tid & 15));
      const int k = k0 + (ORI == LAY_N ? (tid & 127) : 16 * i + (tid >> 4));
      vw[i] = 0.f;
      if (k < K && u < NU) vw[i] = ORI == LAY_N ? W[(size_t)u * ncol + k] : W[(size_t)k * ncol + u];
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += LAY_KC) {
    if (k0) __syncthreads();
#pragma unroll
    for (int i = 0; i < LAY_IN; ++i) sIn[(4 * i + wv) * LAY_IS + lane] = vi[i];
#pragma unroll
    for (int i = 0; i < LAY_WN; ++i) {
      if (ORI == LAY_N)
        sW[(2 * i + (tid >> 7)) * LAY_WS + (tid & 127)] = vw[i];
      else
        sW[(tid & 15) * LAY_WS + 16 * i + (tid >> 4)] = vw[i];
    }
    __syncthreads();
    if (k0 + LAY_KC < K) fetch(k0 + LAY_KC);
    // whole k blocks of 4, the k past the width staged as zeros; LAY_KC / 4 is a multiple of FIT_PS, so k block c
    // of a chunk goes to accumulator c mod 4 of the whole sum
    const float* pa = sW + fu * LAY_WS + fk;
    const float* pb = sIn + fk * LAY_IS + wv * 16 + fu;
    const int nb = (min(LAY_KC, K - k0) + 3) >> 2;
    for (int c = 0; c < nb; c += FIT_PS) {
#pragma unroll
      for (int p = 0; p < FIT_PS; ++p)
        if (c + p < nb)
          acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[(c + p) * 4], pb[(c + p) * 4 * LAY_IS], acc[p], 0, 0, 0);
    }
  }

  // the C tile: column (row of the batch) = lane & 15, row (unit) = 4 (lane >> 4) + register
  const int row = tile * FIT_ROWS + wv * 16 + fu;
  const bool live = row < a.B;
  const int L = a.L, nx = a.n[L + 1];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j = u0 + fk * 4 + g;
    if (j >= NU) continue;
    const float s = (acc[0][g] + acc[1][g]) + (acc[2][g] + acc[3][g]);
    const size_t o = (size_t)j * R + row;
    if (EPI == LAY_ACT) {
      float v, d;
      fit_act<DPI_ACT_ELU>(s + a.b[l - 1][j], v, d);
      ws[a.offA[l] + o] = v;
      ws[a.offP[l] + o] = d;
    } else if (EPI == LAY_OUT) {
      ws[a.offN + o] = s + a.b[l - 1][j];
    } else if (EPI == LAY_ADJ) {
      ws[a.offZ[l - 1] + o] = s;
      ws[a.offD[l - 1] + o] = s * ws[a.offP[l - 1] + o];
    } else if (EPI == LAY_Q) {
      if (live) a.q[(size_t)row * nx + (j - CORE_NT)] = ws[a.offN + (size_t)(j - CORE_NT) * R + row] + s;
    } else if (EPI == LAY_TAN) {
      const float d = ws[a.offP[l] + o];
      ws[a.offLB[l] + o] = s * d;
      ws[a.offZ[l] + o] = s * ws[a.offZ[l] + o] * fit_act_d2<DPI_ACT_ELU>(ws[a.offA[l] + o], d);
    } else if (EPI == LAY_REV) {
      float zb = s * ws[a.offP[l - 1] + o];
      if (a.grad) zb += ws[a.offZ[l - 1] + o];
      ws[a.offZ[l - 1] + o] = zb;
    } else {
      if (live) a.dtau[(size_t)row * CORE_NT + j] = s;
    }
  }
}

// The three launches below that are no product take 16 units x 64 rows per workgroup, 4 elements a thread with
// their loads in flight together: element e of a thread is row (tid + 256 e) >> 4, unit 16 blockIdx.y + (tid & 15).

// a_0 = (tau, x) parked, dead rows as zeros.  Grid (tiles, ceil(n0 / 16)), LAY_NTH threads.
__global__ __launch_bounds__(LAY_NTH) void k_fit_layers_a0(const FitCoreArgs a) {
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int n0 = a.n[0];
  const int i = blockIdx.y * LAY_UT + (threadIdx.x & 15);
  float* A0 = a.ws + a.offA[0];
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int gr = blockIdx.x * FIT_ROWS + ((threadIdx.x + LAY_NTH * e) >> 4);
    v[e] = 0.f;
    if (gr < a.B && i < n0)
      v[e] = i < CORE_NT ? a.tau[(size_t)gr * a.taustride + i] : a.x[(size_t)gr * a.xstride + (i - CORE_NT)];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i < n0) A0[(size_t)i * R + blockIdx.x * FIT_ROWS + ((threadIdx.x + LAY_NTH * e) >> 4)] = v[e];
}

// sp = x . N, units in order as 4 partial sums (k_fit_core_fwd's sum).  Grid (tiles), 64 threads: lane = row.
__global__ __launch_bounds__(FIT_ROWS) void k_fit_layers_sp(const FitCoreArgs a) {
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int row = blockIdx.x * FIT_ROWS + threadIdx.x;
  const int nx = a.n[a.L + 1];
  const float* __restrict__ X = a.ws + a.offD[a.L + 1] + row;
  const float* __restrict__ N = a.ws + a.offN + row;
  float s[FIT_PS] = {0.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j + 8 <= nx; j += 8) {
    float xv[8], nv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      xv[t] = X[(size_t)(j + t) * R];
      nv[t] = N[(size_t)(j + t) * R];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) s[t & (FIT_PS - 1)] = fmaf(xv[t], nv[t], s[t & (FIT_PS - 1)]);
  }
  for (; j < nx; ++j) s[j & (FIT_PS - 1)] = fmaf(X[(size_t)j * R], N[(size_t)j * R], s[j & (FIT_PS - 1)]);
  if (row < a.B) a.sp[row] = (s[0] + s[1]) + (s[2] + s[3]);
}

// The seeds of the backward: lambdabar_0 = (0_tau, r) where r is given, and zbar_{L+1} = e x (+ r); dead rows
// are zeros.  Grid (tiles, ceil(n0 / 16)), LAY_NTH threads: unit i of lambdabar_0 and, where i < nx, of zbar_{L+1}.
__global__ __launch_bounds__(LAY_NTH) void k_fit_layers_seed(const FitCoreArgs a) {
  const size_t R = (size_t)a.tiles * FIT_ROWS;
  const int L = a.L;
  const int n0 = a.n[0], nx = a.n[L + 1];
  const int i = blockIdx.y * LAY_UT + (threadIdx.x & 15);
  float* LB0 = a.ws + a.offLB[0];
  float* ZO = a.ws + a.offZ[L + 1];
  const float* X = a.ws + a.offD[L + 1];
  float lb[4], zo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int gr = blockIdx.x * FIT_ROWS + ((threadIdx.x + LAY_NTH * e) >> 4);
    lb[e] = zo[e] = 0.f;
    if (gr < a.B) {
      if (a.grad && i >= CORE_NT && i < n0) lb[e] = a.r[(size_t)gr * nx + (i - CORE_NT)];
      if (i < nx) {
        zo[e] = a.e[gr] * X[(size_t)i * R + gr];
        if (a.grad) zo[e] += a.r[(size_t)gr * nx + i];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const size_t gr = (size_t)blockIdx.x * FIT_ROWS + ((threadIdx.x + LAY_NTH * e) >> 4);
    if (a.grad && i < n0) LB0[(size_t)i * R + gr] = lb[e];
    if (i < nx) ZO[(size_t)i * R + gr] = zo[e];
  }
}

}  // namespace dpi
