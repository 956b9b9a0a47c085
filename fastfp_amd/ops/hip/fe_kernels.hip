// fastfp_amd Fe sky-assembly kernels for AMD Instinct MI355X (gfx950).
//
// Input: the five corrected per-pulsar products
//   prods (P, D, 5, F) = [ss, cc, sc, sr, cr]   (trsm_prods output)
// and the antenna table ant (nsky, P, 2) = [F+, Fx].  Per (sky, draw,
// frequency) point the Fe statistic needs 13 sums over pulsars,
//   M = sum_p {F+^2, F+Fx, Fx^2} x {ss, sc, cc}   (10 distinct entries)
//   N = sum_p {F+, Fx} x {sr, cr}
// then Fe = 1/2 N^T M^-1 N (4x4).  The sums are a small GEMM with K = P:
// rows = sky points, columns = flattened (d, f), so they run on
// v_mfma_f64_16x16x4f64 with P zero-padded to a multiple of 4.
//
// Layout (same as trsm_fp_kernel, tools/mfma_probe.hip):
//   a      = A[row lane&15][k lane>>4]
//   b      = B[k lane>>4][col lane&15]
//   acc[v] = C[row 4v + (lane>>4)][col lane&15]
// so after the K loop a lane holds all 13 sums of its four (sky, column)
// points and the 4x4 factorisation + solve run in its own registers.
//
// Blocking: one workgroup (4 waves) owns ONE 16-column tile for the
// whole sky.  The operand with reuse is the product tile (read once per
// sky tile, 48x at nsky = 768), so it is staged ONCE per block into LDS
// as Bs[5][Kp][16] — a wave's b read is 4 rows x 16 contiguous doubles,
// conflict-free.  Wave w walks sky tiles w, w+4, ...; its a operands
// come straight from the (L2-resident, < 1 MB) antenna table and the
// three coefficient products are formed in registers: a 64-sky round of
// coefficient planes would need 5 x Kp x 64 doubles of LDS (174 KB at
// P = 67) next to the resident product tile, and no two lanes of a
// block share a coefficient value anyway.
//
// fe_skymax keeps the running sky maximum per lane, reduces the four
// row groups by shuffles and the four waves through 16 LDS slots: a
// column is owned by exactly one block, there are no atomics, and the
// result is bitwise reproducible.  Ties go to the lowest sky index.

#include <hip/hip_runtime.h>
#include <math.h>

#include "launchers.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#define FE_WAVES 4
#define FE_THREADS (FE_WAVES * 64)
#define FE_RCOND 1e-12

// the 13 (coefficient, product) sums of one point
enum {
  S_P2SS = 0, S_P2SC, S_P2CC,  // F+^2  x ss, sc, cc
  S_PXSS, S_PXSC, S_PXCC,      // F+Fx  x ss, sc, cc
  S_X2SS, S_X2SC, S_X2CC,      // Fx^2  x ss, sc, cc
  S_PSR, S_PCR,                // F+    x sr, cr
  S_XSR, S_XCR,                // Fx    x sr, cr
  FE_NSUM
};

static __device__ __forceinline__ bool fe_pivot_ok(double s, double mjj) {
  // false for s <= rcond * M_jj, NaN and +-inf
  return (s > FE_RCOND * mjj) && (s < INFINITY);
}

// Fe of one point from its 13 sums: LDL^T of the 4x4 M (the pivots d_j
// are the squared Cholesky diagonal, so the degeneracy test is the
// Cholesky pivot test), unit-lower forward solve z = L^-1 N, and
// Fe = 1/2 sum_j z_j^2 / d_j = 1/2 y^T y with y the Cholesky solve.
// Returns false (point skipped) on a degenerate or non-finite pivot.
static __device__ __forceinline__ bool fe_point(const double* s, double* fe) {
  // filters: 0 = F+ sin, 1 = F+ cos, 2 = Fx sin, 3 = Fx cos
  const double m00 = s[S_P2SS], m01 = s[S_P2SC], m02 = s[S_PXSS];
  const double m03 = s[S_PXSC], m11 = s[S_P2CC], m12 = s[S_PXSC];
  const double m13 = s[S_PXCC], m22 = s[S_X2SS], m23 = s[S_X2SC];
  const double m33 = s[S_X2CC];

  const double d0 = m00;
  if (!fe_pivot_ok(d0, m00)) return false;
  const double i0 = 1.0 / d0;
  const double l10 = m01 * i0, l20 = m02 * i0, l30 = m03 * i0;

  const double d1 = fma(-l10, m01, m11);
  if (!fe_pivot_ok(d1, m11)) return false;
  const double i1 = 1.0 / d1;
  const double t21 = fma(-l20, m01, m12);
  const double t31 = fma(-l30, m01, m13);
  const double l21 = t21 * i1, l31 = t31 * i1;

  const double d2 = fma(-l21, t21, fma(-l20, m02, m22));
  if (!fe_pivot_ok(d2, m22)) return false;
  const double i2 = 1.0 / d2;
  const double t32 = fma(-l31, t21, fma(-l30, m02, m23));
  const double l32 = t32 * i2;

  const double d3 = fma(-l32, t32, fma(-l31, t31, fma(-l30, m03, m33)));
  if (!fe_pivot_ok(d3, m33)) return false;
  const double i3 = 1.0 / d3;

  const double z0 = s[S_PSR];
  const double z1 = fma(-l10, z0, s[S_PCR]);
  const double z2 = fma(-l21, z1, fma(-l20, z0, s[S_XSR]));
  const double z3 = fma(-l32, z2, fma(-l31, z1, fma(-l30, z0, s[S_XCR])));
  *fe = 0.5 * fma(z3 * z3, i3, fma(z2 * z2, i2, fma(z1 * z1, i1, z0 * z0 * i0)));
  return true;
}

// grid = ceil(D*F / 16) column tiles;  block = 256 (4 waves)
// dynamic LDS = 5 * Kp * 16 doubles (Kp = P rounded up to 4)
// SKYMAX = false: fe (D, nsky, F), NaN at skipped points
// SKYMAX = true : femax/argmax/nskip (D, F)
// Occupancy target 3 waves/SIMD: 13 accumulator quads are 104 VGPRs, so
// 4 waves/SIMD (128) cannot hold them; at 3 the compiler keeps them in
// VGPRs (150 total, no AGPR copies, no scratch) and three blocks' product
// tiles (43.5 KB each at P = 67) fit the 160 KB LDS.
template <bool SKYMAX>
__global__ __launch_bounds__(FE_THREADS, 3) void fe_sky_kernel(
    const double* __restrict__ prods /*(P, D, 5, F)*/,
    const double* __restrict__ ant /*(nsky, P, 2)*/, int P, int D, int F,
    int nsky, double* __restrict__ fe /*(D, nsky, F)*/,
    double* __restrict__ femax /*(D, F)*/, int* __restrict__ argmax /*(D, F)*/,
    int* __restrict__ nskip /*(D, F)*/) {
  extern __shared__ double Bs[];  // [5][Kp][16]
  __shared__ double red_v[FE_WAVES][16];
  __shared__ int red_i[FE_WAVES][16];
  __shared__ int red_n[FE_WAVES][16];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int li = lane & 15;  // a row (sky) / b,acc column
  const int lk = lane >> 4;  // k index / acc row group
  const int Kp = (P + 3) & ~3;
  const int nks = Kp >> 2;
  const long NC = (long)D * F;
  const long n0 = (long)blockIdx.x * 16;

  // stage the product tile: Bs[c][k][j] = prods[k][d][c][f] of column
  // n0 + j, zero for k >= P and for columns past D*F.  j is the fastest
  // thread index, so the loads are contiguous in f.
  {
    const int j = tid & 15;
    const long n = n0 + j;
    const bool cok = n < NC;
    const long d = cok ? n / F : 0;
    const long f = cok ? n % F : 0;
    const long cbase = d * 5 * F + f;
    for (int r = tid >> 4; r < 5 * Kp; r += FE_THREADS / 16) {
      const int k = r / 5;
      const int c = r - 5 * k;
      double v = 0.0;
      if (cok && k < P) v = prods[(long)k * D * 5 * F + cbase + (long)c * F];
      Bs[((long)c * Kp + k) * 16 + j] = v;
    }
  }
  __syncthreads();

  const long ncol = n0 + li;  // this lane's column
  const bool colok = ncol < NC;
  const long cd = colok ? ncol / F : 0;
  const long cf = colok ? ncol % F : 0;

  double best = -INFINITY;
  int besti = -1;
  int nsk = 0;

  const int nst = (nsky + 15) >> 4;
  for (int st = wv; st < nst; st += FE_WAVES) {
    const int s0 = st << 4;
    const int arow = s0 + li;  // the sky row this lane feeds as a
    const bool aok = arow < nsky;
    const double* ap = ant + (long)(aok ? arow : 0) * P * 2;

    f64x4 acc[FE_NSUM];
#pragma unroll
    for (int i = 0; i < FE_NSUM; ++i) acc[i] = f64x4{0, 0, 0, 0};

    // software-prefetched antenna pair of the next k-step
    double fp = 0.0, fx = 0.0;
    if (aok && lk < P) {
      fp = ap[2 * lk];
      fx = ap[2 * lk + 1];
    }
    for (int ks = 0; ks < nks; ++ks) {
      const int k = 4 * ks + lk;
      double nfp = 0.0, nfx = 0.0;
      if (aok && k + 4 < P) {
        nfp = ap[2 * (k + 4)];
        nfx = ap[2 * (k + 4) + 1];
      }
      const double p2 = fp * fp, px = fp * fx, x2 = fx * fx;
      const double bss = Bs[((long)0 * Kp + k) * 16 + li];
      const double bcc = Bs[((long)1 * Kp + k) * 16 + li];
      const double bsc = Bs[((long)2 * Kp + k) * 16 + li];
      const double bsr = Bs[((long)3 * Kp + k) * 16 + li];
      const double bcr = Bs[((long)4 * Kp + k) * 16 + li];
      acc[S_P2SS] = MFMA_F64(p2, bss, acc[S_P2SS]);
      acc[S_P2SC] = MFMA_F64(p2, bsc, acc[S_P2SC]);
      acc[S_P2CC] = MFMA_F64(p2, bcc, acc[S_P2CC]);
      acc[S_PXSS] = MFMA_F64(px, bss, acc[S_PXSS]);
      acc[S_PXSC] = MFMA_F64(px, bsc, acc[S_PXSC]);
      acc[S_PXCC] = MFMA_F64(px, bcc, acc[S_PXCC]);
      acc[S_X2SS] = MFMA_F64(x2, bss, acc[S_X2SS]);
      acc[S_X2SC] = MFMA_F64(x2, bsc, acc[S_X2SC]);
      acc[S_X2CC] = MFMA_F64(x2, bcc, acc[S_X2CC]);
      acc[S_PSR] = MFMA_F64(fp, bsr, acc[S_PSR]);
      acc[S_PCR] = MFMA_F64(fp, bcr, acc[S_PCR]);
      acc[S_XSR] = MFMA_F64(fx, bsr, acc[S_XSR]);
      acc[S_XCR] = MFMA_F64(fx, bcr, acc[S_XCR]);
      fp = nfp;
      fx = nfx;
    }

    // per-lane epilogue: the four (sky 4v + lk, column li) points
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int sky = s0 + 4 * v + lk;
      if (!colok || sky >= nsky) continue;
      double s[FE_NSUM];
#pragma unroll
      for (int i = 0; i < FE_NSUM; ++i) s[i] = acc[i][v];
      double val = 0.0;
      const bool ok = fe_point(s, &val) && (fabs(val) < INFINITY);
      if constexpr (SKYMAX) {
        if (!ok) {
          ++nsk;
        } else if (val > best) {  // sky ascends per lane: first max stays
          best = val;
          besti = sky;
        }
      } else {
        fe[(cd * nsky + sky) * F + cf] = ok ? val : NAN;
      }
    }
  }

  if constexpr (SKYMAX) {
    // row groups lk = 0..3 share the column: lanes +16, +32
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const double ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(besti, off, 64);
      nsk += __shfl_xor(nsk, off, 64);
      if (ov > best || (ov == best && oi >= 0 && (besti < 0 || oi < besti))) {
        best = ov;
        besti = oi;
      }
    }
    if (lk == 0) {
      red_v[wv][li] = best;
      red_i[wv][li] = besti;
      red_n[wv][li] = nsk;
    }
    __syncthreads();
    if (wv == 0 && lk == 0 && colok) {
#pragma unroll
      for (int w = 1; w < FE_WAVES; ++w) {
        const double ov = red_v[w][li];
        const int oi = red_i[w][li];
        nsk += red_n[w][li];
        if (ov > best || (ov == best && oi >= 0 && (besti < 0 || oi < besti))) {
          best = ov;
          besti = oi;
        }
      }
      femax[ncol] = best;
      argmax[ncol] = besti;
      nskip[ncol] = nsk;
    }
  }
}

// fe_point with the back substitution: the same LDL^T and forward solve,
// operation for operation (kept apart from fe_point so the sky kernels
// compile exactly as before), then a = L^-T D^-1 z.  a[0..3] multiply
// the filters F+ sin, F+ cos, Fx sin, Fx cos.
static __device__ __forceinline__ bool fe_point_amps(const double* s,
                                                     double* fe, double* a) {
  const double m00 = s[S_P2SS], m01 = s[S_P2SC], m02 = s[S_PXSS];
  const double m03 = s[S_PXSC], m11 = s[S_P2CC], m12 = s[S_PXSC];
  const double m13 = s[S_PXCC], m22 = s[S_X2SS], m23 = s[S_X2SC];
  const double m33 = s[S_X2CC];

  const double d0 = m00;
  if (!fe_pivot_ok(d0, m00)) return false;
  const double i0 = 1.0 / d0;
  const double l10 = m01 * i0, l20 = m02 * i0, l30 = m03 * i0;

  const double d1 = fma(-l10, m01, m11);
  if (!fe_pivot_ok(d1, m11)) return false;
  const double i1 = 1.0 / d1;
  const double t21 = fma(-l20, m01, m12);
  const double t31 = fma(-l30, m01, m13);
  const double l21 = t21 * i1, l31 = t31 * i1;

  const double d2 = fma(-l21, t21, fma(-l20, m02, m22));
  if (!fe_pivot_ok(d2, m22)) return false;
  const double i2 = 1.0 / d2;
  const double t32 = fma(-l31, t21, fma(-l30, m02, m23));
  const double l32 = t32 * i2;

  const double d3 = fma(-l32, t32, fma(-l31, t31, fma(-l30, m03, m33)));
  if (!fe_pivot_ok(d3, m33)) return false;
  const double i3 = 1.0 / d3;

  const double z0 = s[S_PSR];
  const double z1 = fma(-l10, z0, s[S_PCR]);
  const double z2 = fma(-l21, z1, fma(-l20, z0, s[S_XSR]));
  const double z3 = fma(-l32, z2, fma(-l31, z1, fma(-l30, z0, s[S_XCR])));
  *fe = 0.5 * fma(z3 * z3, i3, fma(z2 * z2, i2, fma(z1 * z1, i1, z0 * z0 * i0)));

  // L^T a = D^-1 z, from the last row up
  const double a3 = z3 * i3;
  const double a2 = fma(-l32, a3, z2 * i2);
  const double a1 = fma(-l31, a3, fma(-l21, a2, z1 * i1));
  const double a0 = fma(-l30, a3, fma(-l20, a2, fma(-l10, a1, z0 * i0)));
  a[0] = a0;
  a[1] = a1;
  a[2] = a2;
  a[3] = a3;
  return true;
}

#define FE_AMPS_THREADS 64

// Maximum-likelihood amplitudes a = M^-1 N at ONE sky index per column.
// grid = ceil(D*F / 64);  block = 64: one thread per column n = d*F + f,
// so the five product loads of a k-step are contiguous in f across
// lanes.  The 13 sums run as a serial k = 0..P-1 FMA chain (fixed order:
// bitwise reproducible); the antenna pair comes from row idx[n] of the
// L2-resident table.  No LDS, no barriers, no atomics, no cap on P.
// status: 0 solved; 1 degenerate or non-finite pivot (fe_pivot_ok);
// 2 idx[n] outside [0, nsky) — the antenna table is not read.  amps and
// fe are NaN wherever status != 0.
__global__ __launch_bounds__(FE_AMPS_THREADS) void fe_amps_kernel(
    const double* __restrict__ prods /*(P, D, 5, F)*/,
    const double* __restrict__ ant /*(nsky, P, 2)*/,
    const int* __restrict__ idx /*(D, F)*/, int P, int D, int F, int nsky,
    double* __restrict__ amps /*(D, F, 4)*/, double* __restrict__ fe /*(D, F)*/,
    int* __restrict__ status /*(D, F)*/) {
  const long NC = (long)D * F;
  const long n = (long)blockIdx.x * FE_AMPS_THREADS + threadIdx.x;
  if (n >= NC) return;
  const long d = n / F;
  const long f = n - d * F;
  const int row = idx[n];

  double a[4] = {NAN, NAN, NAN, NAN};
  double val = NAN;
  int st = 2;
  if (row >= 0 && row < nsky) {
    const double* ap = ant + (long)row * P * 2;
    const double* pp = prods + d * 5 * F + f;
    const long pstride = (long)D * 5 * F;
    double s[FE_NSUM];
#pragma unroll
    for (int i = 0; i < FE_NSUM; ++i) s[i] = 0.0;
    for (int k = 0; k < P; ++k) {
      const double fp = ap[2 * k], fx = ap[2 * k + 1];
      const double* q = pp + (long)k * pstride;
      const double bss = q[0], bcc = q[F], bsc = q[2 * (long)F];
      const double bsr = q[3 * (long)F], bcr = q[4 * (long)F];
      const double p2 = fp * fp, px = fp * fx, x2 = fx * fx;
      s[S_P2SS] = fma(p2, bss, s[S_P2SS]);
      s[S_P2SC] = fma(p2, bsc, s[S_P2SC]);
      s[S_P2CC] = fma(p2, bcc, s[S_P2CC]);
      s[S_PXSS] = fma(px, bss, s[S_PXSS]);
      s[S_PXSC] = fma(px, bsc, s[S_PXSC]);
      s[S_PXCC] = fma(px, bcc, s[S_PXCC]);
      s[S_X2SS] = fma(x2, bss, s[S_X2SS]);
      s[S_X2SC] = fma(x2, bsc, s[S_X2SC]);
      s[S_X2CC] = fma(x2, bcc, s[S_X2CC]);
      s[S_PSR] = fma(fp, bsr, s[S_PSR]);
      s[S_PCR] = fma(fp, bcr, s[S_PCR]);
      s[S_XSR] = fma(fx, bsr, s[S_XSR]);
      s[S_XCR] = fma(fx, bcr, s[S_XCR]);
    }
    double v = 0.0, x[4];
    const bool ok = fe_point_amps(s, &v, x) && (fabs(v) < INFINITY) &&
                    (fabs(x[0]) < INFINITY) && (fabs(x[1]) < INFINITY) &&
                    (fabs(x[2]) < INFINITY) && (fabs(x[3]) < INFINITY);
    st = ok ? 0 : 1;
    if (ok) {
      val = v;
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = x[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) amps[4 * n + i] = a[i];
  fe[n] = val;
  status[n] = st;
}

// ---------------------------------------------------------------------
// Null distribution of the sky maximum (docs/DESIGN.md section 13).
//
// Under noise alone (sr, cr)_p ~ N(0, [[ss, sc], [sc, cc]]_p), so one
// realisation of a column (d, f) is n_p = L_p z_p with L_p the 2x2
// Cholesky factor of that block (lfac) and z_p a standard-normal pair.
// M does not depend on the realisation: fe_mfac_kernel factors it ONCE
// per (column, sky) and fe_null_kernel only forms the four N sums,
//   rows = sky, columns = realisations, K = P,
// and pushes them through the stored factor.
// ---------------------------------------------------------------------

// the ten numbers of M = L D L^T that the forward solve reads
enum {
  FC_L10 = 0, FC_L20, FC_L30, FC_L21, FC_L31, FC_L32,
  FC_I0, FC_I1, FC_I2, FC_I3,
  FE_NFAC
};

// The LDL^T of fe_point, operation for operation, on the nine M sums
// s[S_P2SS .. S_X2CC] (kept apart from fe_point so the sky kernels
// compile exactly as before).  Returns false on the pivots fe_point
// rejects.
static __device__ __forceinline__ bool fe_point_factor(const double* s,
                                                       double* fc) {
  const double m00 = s[S_P2SS], m01 = s[S_P2SC], m02 = s[S_PXSS];
  const double m03 = s[S_PXSC], m11 = s[S_P2CC], m12 = s[S_PXSC];
  const double m13 = s[S_PXCC], m22 = s[S_X2SS], m23 = s[S_X2SC];
  const double m33 = s[S_X2CC];

  const double d0 = m00;
  if (!fe_pivot_ok(d0, m00)) return false;
  const double i0 = 1.0 / d0;
  const double l10 = m01 * i0, l20 = m02 * i0, l30 = m03 * i0;

  const double d1 = fma(-l10, m01, m11);
  if (!fe_pivot_ok(d1, m11)) return false;
  const double i1 = 1.0 / d1;
  const double t21 = fma(-l20, m01, m12);
  const double t31 = fma(-l30, m01, m13);
  const double l21 = t21 * i1, l31 = t31 * i1;

  const double d2 = fma(-l21, t21, fma(-l20, m02, m22));
  if (!fe_pivot_ok(d2, m22)) return false;
  const double i2 = 1.0 / d2;
  const double t32 = fma(-l31, t21, fma(-l30, m02, m23));
  const double l32 = t32 * i2;

  const double d3 = fma(-l32, t32, fma(-l31, t31, fma(-l30, m03, m33)));
  if (!fe_pivot_ok(d3, m33)) return false;
  const double i3 = 1.0 / d3;

  fc[FC_L10] = l10;
  fc[FC_L20] = l20;
  fc[FC_L30] = l30;
  fc[FC_L21] = l21;
  fc[FC_L31] = l31;
  fc[FC_L32] = l32;
  fc[FC_I0] = i0;
  fc[FC_I1] = i1;
  fc[FC_I2] = i2;
  fc[FC_I3] = i3;
  return true;
}

// The M factors of every (column, sky) point: the blocking, staging and
// K loop of fe_sky_kernel with the nine M sums only (same a and b
// values, same k order: the sums are bitwise those of fe_skymax), then
// fe_point_factor per lane.
// grid = ceil(D*F / 16);  block = 256;  dynamic LDS = 3 * Kp * 16 doubles
// fac (D*F, nsky, FE_NFAC); a skipped point is ten NaNs (FC_I0 is the
// flag fe_null_kernel tests).
__global__ __launch_bounds__(FE_THREADS, 4) void fe_mfac_kernel(
    const double* __restrict__ prods /*(P, D, 5, F)*/,
    const double* __restrict__ ant /*(nsky, P, 2)*/, int P, int D, int F,
    int nsky, double* __restrict__ fac /*(D*F, nsky, FE_NFAC)*/) {
  extern __shared__ double Bs[];  // [3][Kp][16]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int li = lane & 15;
  const int lk = lane >> 4;
  const int Kp = (P + 3) & ~3;
  const int nks = Kp >> 2;
  const long NC = (long)D * F;
  const long n0 = (long)blockIdx.x * 16;

  {
    const int j = tid & 15;
    const long n = n0 + j;
    const bool cok = n < NC;
    const long d = cok ? n / F : 0;
    const long f = cok ? n % F : 0;
    const long cbase = d * 5 * F + f;
    for (int r = tid >> 4; r < 3 * Kp; r += FE_THREADS / 16) {
      const int k = r / 3;
      const int c = r - 3 * k;
      double v = 0.0;
      if (cok && k < P) v = prods[(long)k * D * 5 * F + cbase + (long)c * F];
      Bs[((long)c * Kp + k) * 16 + j] = v;
    }
  }
  __syncthreads();

  const long ncol = n0 + li;
  const bool colok = ncol < NC;

  const int nst = (nsky + 15) >> 4;
  for (int st = wv; st < nst; st += FE_WAVES) {
    const int s0 = st << 4;
    const int arow = s0 + li;
    const bool aok = arow < nsky;
    const double* ap = ant + (long)(aok ? arow : 0) * P * 2;

    f64x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = f64x4{0, 0, 0, 0};

    double fp = 0.0, fx = 0.0;
    if (aok && lk < P) {
      fp = ap[2 * lk];
      fx = ap[2 * lk + 1];
    }
    for (int ks = 0; ks < nks; ++ks) {
      const int k = 4 * ks + lk;
      double nfp = 0.0, nfx = 0.0;
      if (aok && k + 4 < P) {
        nfp = ap[2 * (k + 4)];
        nfx = ap[2 * (k + 4) + 1];
      }
      const double p2 = fp * fp, px = fp * fx, x2 = fx * fx;
      const double bss = Bs[((long)0 * Kp + k) * 16 + li];
      const double bcc = Bs[((long)1 * Kp + k) * 16 + li];
      const double bsc = Bs[((long)2 * Kp + k) * 16 + li];
      acc[S_P2SS] = MFMA_F64(p2, bss, acc[S_P2SS]);
      acc[S_P2SC] = MFMA_F64(p2, bsc, acc[S_P2SC]);
      acc[S_P2CC] = MFMA_F64(p2, bcc, acc[S_P2CC]);
      acc[S_PXSS] = MFMA_F64(px, bss, acc[S_PXSS]);
      acc[S_PXSC] = MFMA_F64(px, bsc, acc[S_PXSC]);
      acc[S_PXCC] = MFMA_F64(px, bcc, acc[S_PXCC]);
      acc[S_X2SS] = MFMA_F64(x2, bss, acc[S_X2SS]);
      acc[S_X2SC] = MFMA_F64(x2, bsc, acc[S_X2SC]);
      acc[S_X2CC] = MFMA_F64(x2, bcc, acc[S_X2CC]);
      fp = nfp;
      fx = nfx;
    }

#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int sky = s0 + 4 * v + lk;
      if (!colok || sky >= nsky) continue;
      double s[9], fc[FE_NFAC];
#pragma unroll
      for (int i = 0; i < 9; ++i) s[i] = acc[i][v];
      const bool ok = fe_point_factor(s, fc);
      double* out = fac + (ncol * nsky + sky) * FE_NFAC;
#pragma unroll
      for (int i = 0; i < FE_NFAC; ++i) out[i] = ok ? fc[i] : NAN;
    }
  }
}

// Null sky maximum.  One workgroup (4 waves) owns ONE column (d, f) and
// RT tiles of 16 realisations; grid = D*F * ngrp, ngrp = ceil(R / 16 RT),
// the groups of a column adjacent so they share its factors in L2.
// The realisations n = L z are formed while staging (z is contiguous in
// R: a wave reads consecutive doubles) into Ns[2][RT][Kp][16], the
// conflict-free b layout of fe_sky_kernel per tile.  Wave w walks sky
// tiles w, w+4, ...: ONE a load feeds 4 RT MFMAs per k-step, and the ten
// factor numbers of a lane's four sky rows are read once per sky tile
// for all RT tiles.  The forward solve is fe_point's on the stored
// factor.  A realisation is one b column and one accumulator column: its
// result does not depend on RT, on its tile or on its block.
// dynamic LDS = 2 * RT * Kp * 16 doubles
template <int RT>
__global__ __launch_bounds__(FE_THREADS, RT == 4 ? 2 : 4) void fe_null_kernel(
    const double* __restrict__ ant /*(nsky, P, 2)*/,
    const double* __restrict__ lfac /*(D*F, P, 3)*/,
    const double* __restrict__ z /*(D*F, P, 2, R)*/,
    const double* __restrict__ fac /*(D*F, nsky, FE_NFAC)*/, int P, int nsky,
    int R, int ngrp, double* __restrict__ femax /*(D*F, R)*/,
    int* __restrict__ argmax /*(D*F, R)*/, int* __restrict__ nskip /*(D*F)*/) {
  extern __shared__ double Ns[];  // [2][RT][Kp][16]
  __shared__ double red_v[FE_WAVES][16 * RT];
  __shared__ int red_i[FE_WAVES][16 * RT];
  __shared__ int red_n[FE_WAVES];

  constexpr int W = 16 * RT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int li = lane & 15;  // a row (sky) / b,acc column (realisation)
  const int lk = lane >> 4;  // k index / acc row group
  const int Kp = (P + 3) & ~3;
  const int nks = Kp >> 2;
  const long col = blockIdx.x / ngrp;
  const int grp = blockIdx.x - (int)(col * ngrp);
  const long r0 = (long)grp * W;

  // stage n_s = l00 z0, n_c = l10 z0 + l11 z1; zero for k >= P, r >= R
  for (int e = tid; e < Kp * W; e += FE_THREADS) {
    const int k = e / W;
    const int j = e - k * W;
    const long r = r0 + j;
    double ns = 0.0, nc = 0.0;
    if (k < P && r < R) {
      const double* lp = lfac + (col * P + k) * 3;
      const double* zp = z + (col * P + k) * 2 * R + r;
      const double z0 = zp[0], z1 = zp[R];
      ns = lp[0] * z0;
      nc = fma(lp[1], z0, lp[2] * z1);
    }
    const long o = ((long)(j >> 4) * Kp + k) * 16 + (j & 15);
    Ns[o] = ns;
    Ns[(long)RT * Kp * 16 + o] = nc;
  }
  __syncthreads();

  double best[RT];
  int besti[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    best[t] = -INFINITY;
    besti[t] = -1;
  }
  int nsk = 0;
  const double* fcol = fac + col * nsky * FE_NFAC;

  const int nst = (nsky + 15) >> 4;
  for (int st = wv; st < nst; st += FE_WAVES) {
    const int s0 = st << 4;
    const int arow = s0 + li;
    const bool aok = arow < nsky;
    const double* ap = ant + (long)(aok ? arow : 0) * P * 2;

    f64x4 acc[4 * RT];
#pragma unroll
    for (int i = 0; i < 4 * RT; ++i) acc[i] = f64x4{0, 0, 0, 0};

    double fp = 0.0, fx = 0.0;
    if (aok && lk < P) {
      fp = ap[2 * lk];
      fx = ap[2 * lk + 1];
    }
    for (int ks = 0; ks < nks; ++ks) {
      const int k = 4 * ks + lk;
      double nfp = 0.0, nfx = 0.0;
      if (aok && k + 4 < P) {
        nfp = ap[2 * (k + 4)];
        nfx = ap[2 * (k + 4) + 1];
      }
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const double bs = Ns[((long)t * Kp + k) * 16 + li];
        const double bc = Ns[((long)(RT + t) * Kp + k) * 16 + li];
        acc[4 * t + 0] = MFMA_F64(fp, bs, acc[4 * t + 0]);
        acc[4 * t + 1] = MFMA_F64(fp, bc, acc[4 * t + 1]);
        acc[4 * t + 2] = MFMA_F64(fx, bs, acc[4 * t + 2]);
        acc[4 * t + 3] = MFMA_F64(fx, bc, acc[4 * t + 3]);
      }
      fp = nfp;
      fx = nfx;
    }

    // per-lane epilogue: sky rows 4v + lk, realisations t * 16 + li
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int sky = s0 + 4 * v + lk;
      if (sky >= nsky) continue;
      const double* fc = fcol + (long)sky * FE_NFAC;
      const double i0 = fc[FC_I0];
      if (!(i0 == i0)) {  // skipped by the pivot rule
        ++nsk;
        continue;
      }
      const double l10 = fc[FC_L10], l20 = fc[FC_L20], l30 = fc[FC_L30];
      const double l21 = fc[FC_L21], l31 = fc[FC_L31], l32 = fc[FC_L32];
      const double i1 = fc[FC_I1], i2 = fc[FC_I2], i3 = fc[FC_I3];
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const double z0 = acc[4 * t + 0][v];
        const double z1 = fma(-l10, z0, acc[4 * t + 1][v]);
        const double z2 = fma(-l21, z1, fma(-l20, z0, acc[4 * t + 2][v]));
        const double z3 =
            fma(-l32, z2, fma(-l31, z1, fma(-l30, z0, acc[4 * t + 3][v])));
        const double val =
            0.5 * fma(z3 * z3, i3, fma(z2 * z2, i2, fma(z1 * z1, i1, z0 * z0 * i0)));
        // sky ascends per lane: the first maximum stays; a non-finite
        // value (non-finite z) never becomes the maximum
        if ((fabs(val) < INFINITY) && val > best[t]) {
          best[t] = val;
          besti[t] = sky;
        }
      }
    }
  }

  // row groups lk = 0..3 share the realisation: lanes +16, +32
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    nsk += __shfl_xor(nsk, off, 64);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const double ov = __shfl_xor(best[t], off, 64);
      const int oi = __shfl_xor(besti[t], off, 64);
      if (ov > best[t] ||
          (ov == best[t] && oi >= 0 && (besti[t] < 0 || oi < besti[t]))) {
        best[t] = ov;
        besti[t] = oi;
      }
    }
  }
  if (lk == 0) {
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      red_v[wv][t * 16 + li] = best[t];
      red_i[wv][t * 16 + li] = besti[t];
    }
    if (li == 0) red_n[wv] = nsk;  // the same count in every column
  }
  __syncthreads();
  if (wv == 0 && lk == 0) {
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      double b = best[t];
      int bi = besti[t];
#pragma unroll
      for (int w = 1; w < FE_WAVES; ++w) {
        const double ov = red_v[w][t * 16 + li];
        const int oi = red_i[w][t * 16 + li];
        if (ov > b || (ov == b && oi >= 0 && (bi < 0 || oi < bi))) {
          b = ov;
          bi = oi;
        }
      }
      const long r = r0 + t * 16 + li;
      if (r < R) {
        femax[col * R + r] = b;
        argmax[col * R + r] = bi;
      }
    }
    if (grp == 0 && li == 0)
      nskip[col] = red_n[0] + red_n[1] + red_n[2] + red_n[3];
  }
}

// Realisation tiles per workgroup of fe_null_kernel when the caller asks
// for none (rtiles = 0): measured in docs/DESIGN.md section 13.
#define FE_NULL_RT 2
// dynamic LDS a workgroup may ask for next to the static reduction slots
#define FE_NULL_LDS_MAX (144 * 1024)

template <int RT>
static hipError_t fe_null_launch(const double* ant, const double* lfac,
                                 const double* z, const double* fac, int P,
                                 long NC, int nsky, int R, double* femax,
                                 int* argmax, int* nskip,
                                 hipStream_t stream) {
  const int Kp = (P + 3) & ~3;
  const size_t lds = (size_t)2 * RT * Kp * 16 * sizeof(double);
  const long ngrp = ((long)R + 16 * RT - 1) / (16 * RT);
  if (NC * ngrp > 0x7fffffffL) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)fe_null_kernel<RT>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(fe_null_kernel<RT>, dim3((unsigned)(NC * ngrp)),
                     dim3(FE_THREADS), lds, stream, ant, lfac, z, fac, P,
                     nsky, R, (int)ngrp, femax, argmax, nskip);
  return hipGetLastError();
}

// ---------------------------------------------------------------------
// Joint null data across frequencies (docs/DESIGN.md section 14).
//
//   n[d, f, p, c, r] = white[p, r, 2f+c] - sum_k rhs[p, k, 2f+c] X[p, d, k, r]
//
// a batched fp64 GEMM over (pulsar, draw) with M = 2F rows (2f+c), N = R
// columns (realisations) and K = mp, in the operand layout at the top of
// this file: a = -rhs[k][row], b = X[k][col], acc = C[row][col].  The
// accumulators START from the white tile (read transposed: white is
// (r, 2f+c) as sbgemm writes it) and the factor's columns enter negated,
// so the MFMA chain IS the subtraction.
//
// One workgroup (4 waves) owns a 64 x 64 tile of one (pulsar, draw): wave
// w the 16 rows 16w.. and all four 16-column tiles, so one a operand
// feeds four MFMAs.  K runs in chunks of 16 staged through LDS as
// As[4][16][16] / Bs[4][16][16] (tile, k, 16): a wave's operand read is 4
// k rows x 16 contiguous doubles, conflict-free as in fe_sky_kernel.  The
// next chunk's 8 doubles per thread are loaded into registers before the
// MFMAs of the current one.  Global loads are contiguous in the row index
// (rhs) and in r (X); rows >= 2F (the last column of rhs is never read)
// and columns >= R are loaded as zero and not stored.  The epilogue
// writes (D, F, P, 2, R) directly: lane l holds column r = l & 15, so a
// row is stored as contiguous 128-byte runs in R.  Fixed k order, no
// atomics: bitwise reproducible.  Static LDS 16 KiB.
// ---------------------------------------------------------------------
#define FND_TILE 64
#define FND_KC 16

__global__ __launch_bounds__(FE_THREADS) void fe_null_data_kernel(
    const double* __restrict__ white /*(P, Rp, ldw)*/,
    const double* __restrict__ rhs /*(P, mp, ldr)*/,
    const double* __restrict__ X /*(P, D, mp, R)*/, int P, int D, int F,
    int R, int mp, long wstride /*Rp * ldw*/, int ldw, int ldr, int mtiles,
    int ntiles, double* __restrict__ out /*(D, F, P, 2, R)*/) {
  __shared__ double As[4][FND_KC][16];
  __shared__ double Bs[4][FND_KC][16];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int li = lane & 15;  // a row within the wave's tile / b,acc column
  const int lk = lane >> 4;  // k index / acc row group
  const int F2 = 2 * F;

  long b = blockIdx.x;
  const int nt = (int)(b % ntiles);
  b /= ntiles;
  const int mt = (int)(b % mtiles);
  b /= mtiles;
  const int d = (int)(b % D);
  const int p = (int)(b / D);
  const int M0 = mt * FND_TILE;
  const int N0 = nt * FND_TILE;

  const double* rp = rhs + (long)p * mp * ldr;
  const double* xp = X + ((long)p * D + d) * mp * R;
  const double* wp = white + (long)p * wstride;

  // staging: element e = tid + 256 i of a chunk is (k = e / 64, j = e % 64)
  const int sj = tid & 63;
  const int sk = tid >> 6;  // k = sk + 4 i
  const bool aok = M0 + sj < F2;
  const bool bok = N0 + sj < R;
  const double* ag = rp + (long)sk * ldr + M0 + sj;
  const double* bg = xp + (long)sk * R + N0 + sj;

  double ra[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = aok ? ag[(long)(4 * i) * ldr] : 0.0;
    rb[i] = bok ? bg[(long)(4 * i) * R] : 0.0;
  }

  // accumulators from the white tile: acc[t][v] = C[row 4v + lk][col li]
  f64x4 acc[4];
  const int row0 = M0 + 16 * wv;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = N0 + 16 * t + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = row0 + 4 * v + lk;
      acc[t][v] = (r < R && row < F2) ? wp[(long)r * ldw + row] : 0.0;
    }
  }

  const int nch = mp / FND_KC;
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[sj >> 4][sk + 4 * i][sj & 15] = -ra[i];
      Bs[sj >> 4][sk + 4 * i][sj & 15] = rb[i];
    }
    __syncthreads();
    if (ch + 1 < nch) {
      const long k0 = (long)(ch + 1) * FND_KC;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = aok ? ag[(k0 + 4 * i) * ldr] : 0.0;
        rb[i] = bok ? bg[(k0 + 4 * i) * R] : 0.0;
      }
    }
#pragma unroll
    for (int ks = 0; ks < FND_KC / 4; ++ks) {
      const double a = As[wv][4 * ks + lk][li];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = MFMA_F64(a, Bs[t][4 * ks + lk][li], acc[t]);
    }
    __syncthreads();
  }

#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int row = row0 + 4 * v + lk;
    if (row >= F2) continue;
    const long f = row >> 1, c = row & 1;
    double* op = out + ((((long)d * F + f) * P + p) * 2 + c) * R;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = N0 + 16 * t + li;
      if (r < R) op[r] = acc[t][v];
    }
  }
}

extern "C" {

int launch_fe_null_data(const double* white, const double* rhs,
                        const double* X, int P, int D, int F, int R, int Rp,
                        int ldw, int mp, double* out, hipStream_t stream) {
  if (P == 0 || D == 0 || F == 0 || R == 0) return (int)hipSuccess;
  if (mp < 16 || mp > 256 || mp % 16 != 0 || Rp < R || ldw < 2 * F)
    return (int)hipErrorInvalidValue;
  const long mtiles = (2L * F + FND_TILE - 1) / FND_TILE;
  const long ntiles = ((long)R + FND_TILE - 1) / FND_TILE;
  const long nblk = (long)P * D * mtiles * ntiles;
  if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fe_null_data_kernel, dim3((unsigned)nblk),
                     dim3(FE_THREADS), 0, stream, white, rhs, X, P, D, F, R,
                     mp, (long)Rp * ldw, ldw, 2 * F + 1, (int)mtiles,
                     (int)ntiles, out);
  return (int)hipGetLastError();
}

// Largest P the resident product tile supports: 5 * Kp * 16 doubles of
// dynamic LDS next to the static reduction slots, within 160 KiB.
int fe_max_pulsars() { return 248; }

static hipError_t fe_launch_common(bool skymax, const double* prods,
                                   const double* ant, int P, int D, int F,
                                   int nsky, double* fe, double* femax,
                                   int* argmax, int* nskip,
                                   hipStream_t stream) {
  const int Kp = (P + 3) & ~3;
  const size_t lds = (size_t)5 * Kp * 16 * sizeof(double);
  const long ntiles = ((long)D * F + 15) / 16;
  if (ntiles == 0 || nsky == 0) return hipSuccess;
  const void* fn = skymax ? (const void*)fe_sky_kernel<true>
                          : (const void*)fe_sky_kernel<false>;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)ntiles), blk(FE_THREADS);
  if (skymax)
    hipLaunchKernelGGL(fe_sky_kernel<true>, grid, blk, lds, stream, prods,
                       ant, P, D, F, nsky, fe, femax, argmax, nskip);
  else
    hipLaunchKernelGGL(fe_sky_kernel<false>, grid, blk, lds, stream, prods,
                       ant, P, D, F, nsky, fe, femax, argmax, nskip);
  return hipGetLastError();
}

int launch_fe_assemble(const double* prods, const double* ant, int P, int D,
                       int F, int nsky, double* fe, hipStream_t stream) {
  return (int)fe_launch_common(false, prods, ant, P, D, F, nsky, fe, nullptr,
                               nullptr, nullptr, stream);
}

int launch_fe_skymax(const double* prods, const double* ant, int P, int D,
                     int F, int nsky, double* femax, int* argmax, int* nskip,
                     hipStream_t stream) {
  return (int)fe_launch_common(true, prods, ant, P, D, F, nsky, nullptr,
                               femax, argmax, nskip, stream);
}

int launch_fe_amplitudes(const double* prods, const double* ant,
                         const int* idx, int P, int D, int F, int nsky,
                         double* amps, double* fe, int* status,
                         hipStream_t stream) {
  const long NC = (long)D * F;
  if (NC == 0) return (int)hipSuccess;
  const long nblk = (NC + FE_AMPS_THREADS - 1) / FE_AMPS_THREADS;
  if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fe_amps_kernel, dim3((unsigned)nblk),
                     dim3(FE_AMPS_THREADS), 0, stream, prods, ant, idx, P, D,
                     F, nsky, amps, fe, status);
  return (int)hipGetLastError();
}

int fe_null_fac_numbers() { return FE_NFAC; }

int launch_fe_mfactor(const double* prods, const double* ant, int P, int D,
                      int F, int nsky, double* fac, hipStream_t stream) {
  const int Kp = (P + 3) & ~3;
  const size_t lds = (size_t)3 * Kp * 16 * sizeof(double);
  const long ntiles = ((long)D * F + 15) / 16;
  if (ntiles == 0 || nsky == 0) return (int)hipSuccess;
  if (ntiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)fe_mfac_kernel,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(fe_mfac_kernel, dim3((unsigned)ntiles), dim3(FE_THREADS),
                     lds, stream, prods, ant, P, D, F, nsky, fac);
  return (int)hipGetLastError();
}

int launch_fe_null_skymax(const double* prods, const double* ant,
                          const double* lfac, const double* z, int P, int D,
                          int F, int nsky, int R, int rtiles, double* fac,
                          double* femax, int* argmax, int* nskip,
                          hipStream_t stream) {
  const long NC = (long)D * F;
  if (NC == 0 || nsky == 0 || R == 0) return (int)hipSuccess;
  if (rtiles != 0 && rtiles != 1 && rtiles != 2 && rtiles != 4)
    return (int)hipErrorInvalidValue;
  int e = launch_fe_mfactor(prods, ant, P, D, F, nsky, fac, stream);
  if (e != 0) return e;
  // no more tiles than R fills, no more than the LDS holds at this P
  int rt = rtiles ? rtiles : FE_NULL_RT;
  const int Kp = (P + 3) & ~3;
  while (rt > 1 && (R <= 8 * rt ||
                    (size_t)2 * rt * Kp * 16 * sizeof(double) > FE_NULL_LDS_MAX))
    rt >>= 1;
  hipError_t err;
  if (rt == 4)
    err = fe_null_launch<4>(ant, lfac, z, fac, P, NC, nsky, R, femax, argmax,
                            nskip, stream);
  else if (rt == 2)
    err = fe_null_launch<2>(ant, lfac, z, fac, P, NC, nsky, R, femax, argmax,
                            nskip, stream);
  else
    err = fe_null_launch<1>(ant, lfac, z, fac, P, NC, nsky, R, femax, argmax,
                            nskip, stream);
  return (int)err;
}

}  // extern "C"
