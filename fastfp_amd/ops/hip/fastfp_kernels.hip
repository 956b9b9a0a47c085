// fastfp_amd fp64 HIP kernels for MI355X (gfx950, CDNA4).
//
// Hand-written from scratch for the restructured Fp-statistic math
// (docs/DESIGN.md) — NOT a port of the reference's JAX
// graph (the reference has zero native code).  The
// implicit XLA op surface being replaced is catalogued in SURVEY.md
// §2.2; each kernel below names the reference call sites it subsumes.
//
// Kernel inventory:
//   sigdots_kernel     — fused sin/cos signal basis + diagonal-weighted
//                        dots sNs/sNr (subsumes fastfp/fastfp.py:78-79 +
//                        utils.py:49-53 elementwise/dot ops)
//   sbgemm_kernel      — MFMA fp64 DGEMM B = T^T (N^-1 S) with the
//                        sin/cos S-panel GENERATED in LDS (never
//                        materialized in HBM) and LDS-staged T panels
//                        (subsumes utils.py:51-52 GEMV batched over all
//                        frequencies)
//   chol_batch_kernel  — batched Cholesky of Sigma = TNT + diag(phi^-1),
//                        assembled in LDS (never materialized in HBM),
//                        MFMA trailing updates, inverted 16x16 diagonal
//                        blocks exported for the solver (subsumes
//                        utils.py:76 + the LU in utils.py:54); the
//                        diagonal comes as a (P,D,m) tensor or is formed
//                        from the strided prior rows in place
//   phi_inv_batch_kernel — the homogeneous prior phi^-1 (P,D,ntm+nf)
//                        from the power-law parameters in one pass, bit
//                        for bit the torch chain of noise.batch_phiinv
//   trsm_fp_kernel     — batched blocked forward-substitution
//                        W = L^-1 [B | TNr] fused with the per-frequency
//                        2x2 Gram/solve/Fp reduction; W lives entirely
//                        in LDS and never touches HBM (subsumes
//                        utils.py:54 + fastfp.py:81-90); its products
//                        mode stores the five corrected products
//                        instead of Fp (the Fe input).  mp <= 128
//   trsm_fp_draws_kernel — the same solve for mp <= 64 with the loop
//                        over draws inside the workgroup: the RHS tile
//                        stays on chip over a slice of draws, Fp is a
//                        plain store (the stacked compressed sweep); its
//                        products mode stores the five products (the
//                        compressed Fe input)
//   trsm_fp_rl_kernel  — right-looking form of the same solve, the
//                        path for 128 < mp <= 256
//   diag_inv_kernel    — inverted 16x16 diagonal blocks of a rocSOLVER
//                        factor (the mp > 128 direct path)
//   sigdots_block_kernel — sigdots for block-diagonal N
//
// Host side (end of the file; declarations in launchers.h): one
// extern "C" launcher per kernel, and two for the solve, each taking an
// `int prods` — launch_trsm (trsm_fp_kernel, trsm_fp_rl_kernel) over
// launch_one_draw<PRODS>, launch_trsm_draws (trsm_fp_draws_kernel) over
// launch_draws<PRODS> — and two for the factor, launch_chol_batch and
// launch_chol_rows over chol_dispatch.
//
// Each launcher below is one dispatch: there are no environment-
// selected variants.  The alternatives that were tried and measured
// neutral or slower (LDS-resident and wave-level solves, a
// double-buffered sbgemm, other grid orders) are recorded in
// docs/TUNING_NOTES.md.
//
// Conventions:
//   wave = 64 lanes (CDNA);  MFMA v_mfma_f64_16x16x4f64:
//     A[i][k]: lane l holds A[i = l&15][k = l>>4]
//     B[k][j]: lane l holds B[k = l>>4][j = l&15]
//     D/C    : lane l holds rows 4*v + (l>>4) (v=0..3), col l&15 (probed: tools/mfma_probe.hip)
//   mp = m padded to a multiple of 16, mp <= 128 for the LDS-resident
//   Cholesky and mp <= 256 for the solve.  Pad rows of Sigma
//   are identity (L pad = I) and pad rows of RHS are zero, so padding
//   never changes results.
//   All reductions have fixed order -> bitwise-deterministic fp64.

#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "launchers.h"

#define FASTFP_MAXMP 128
#define NB 16  // Cholesky/TRSM block size (one MFMA tile)

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
// c - a (x) b: for f64 the last operand is the NEG field, bit 0 negates A
// (printed neg:[1,0,0]); -a*b is exact, so this is MFMA_F64(-a, b, c)
#define MFMA_F64_NEGA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 1)

static __device__ __forceinline__ double wave_reduce_sum(double v) {
  // fixed-order binary tree over the 64-lane wave
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  return v;
}

// ---------------------------------------------------------------------
// sigdots: per-frequency dots  s^T N^-1 s, c^T N^-1 c, s^T N^-1 c,
//          s^T N^-1 r, c^T N^-1 r   (amplitude f^-1/3 omitted: it
//          cancels in Fp — docs/DESIGN.md §2)
// grid.x = F, block = 256
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void sigdots_kernel(
    const double* __restrict__ toas, const double* __restrict__ ninv,
    const double* __restrict__ nr, const double* __restrict__ freqs,
    int ntoa, int F, double* __restrict__ sNs /*(3,F)*/,
    double* __restrict__ sNr /*(2,F)*/) {
  const int f = blockIdx.x;
  if (f >= F) return;
  const double w = 2.0 * M_PI * freqs[f];
  double ss = 0, cc = 0, sc = 0, sr = 0, cr = 0;
  for (int i = threadIdx.x; i < ntoa; i += blockDim.x) {
    double s, c;
    sincos(w * toas[i], &s, &c);
    const double ni = ninv[i];
    const double ri = nr[i];
    ss = fma(s * s, ni, ss);
    cc = fma(c * c, ni, cc);
    sc = fma(s * c, ni, sc);
    sr = fma(s, ri, sr);
    cr = fma(c, ri, cr);
  }
  __shared__ double red[4][5];
  ss = wave_reduce_sum(ss);
  cc = wave_reduce_sum(cc);
  sc = wave_reduce_sum(sc);
  sr = wave_reduce_sum(sr);
  cr = wave_reduce_sum(cr);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = ss; red[wv][1] = cc; red[wv][2] = sc;
    red[wv][3] = sr; red[wv][4] = cr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int v = 0; v < 4; ++v) {
      a0 += red[v][0]; a1 += red[v][1]; a2 += red[v][2];
      a3 += red[v][3]; a4 += red[v][4];
    }
    sNs[f] = a0; sNs[F + f] = a1; sNs[2 * F + f] = a2;
    sNr[f] = a3; sNr[F + f] = a4;
  }
}

// ---------------------------------------------------------------------
// sbgemm: out[j, c] = sum_k T[k, j] * trig_c(toas[k]) * ninv[k]
//   trig_c = sin(2 pi f_{c/2} t) for even c, cos for odd c.
// The S-panel is generated on the fly into LDS (fused signal basis);
// the T-panel is LDS-staged.  Output is the (mp x 2F) RHS block,
// written directly (ksplit==1, ld = ldo) or into per-split partial
// planes (deterministic torch reduction afterwards).
// grid.x = ceil(2F / 64) col tiles, grid.y = ksplit;  block = 512 (8 waves)
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(512) void sbgemm_kernel(
    const double* __restrict__ T /*(ntoa, m) row-major*/,
    const double* __restrict__ toas, const double* __restrict__ ninv,
    const double* __restrict__ freqs, int ntoa, int m, int mp, int F2,
    double* __restrict__ out, long plane_stride, long ldo) {
  // 8 waves: 4 column strips x 2 row halves.  The 4-wave variant held
  // 8 accumulator tiles per wave (64+ AGPR) which capped occupancy at
  // 3 waves/SIMD; splitting the M dim halves the accumulator and lets
  // more waves cover the sincos + LDS latency.
  // grid.z tiles the M dimension in blocks of 128 so the basis size is
  // unbounded (GP-ECORR models run to many hundreds of columns).
  __shared__ double lT[16][FASTFP_MAXMP + 1];
  __shared__ double lS[64][17];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int c0 = blockIdx.x * 64;       // first output column of this tile
  const int mbase = blockIdx.z * FASTFP_MAXMP;  // M-tile origin
  const int mp_loc = min(FASTFP_MAXMP, mp - mbase);
  const int jw = (wv & 3) * 16;         // column strip
  const int rh = wv >> 2;               // row half (0: rows 0-63, 1: 64-127)
  const int rowbase = rh * 64;
  const int nrt_tot = mp_loc >> 4;
  // row tiles this wave owns (half 1 may be empty for small mp)
  const int rt_lo = min(rh * 4, nrt_tot);
  const int rt_hi = min(rt_lo + 4, nrt_tot);

  // K range of this split
  const int ks = gridDim.y;
  const int kchunk = (ntoa + ks - 1) / ks;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(ntoa, kbeg + kchunk);
  double* outp = out + (long)blockIdx.y * plane_stride;

  f64x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f64x4{0, 0, 0, 0};

  for (int k0 = kbeg; k0 < kend; k0 += 16) {
    // stage T panel rows k0..k0+15, cols mbase.. (zero-padded)
    for (int idx = tid; idx < 16 * mp_loc; idx += 512) {
      const int k = idx / mp_loc, j = idx % mp_loc;
      const int gk = k0 + k;
      const int gj = mbase + j;
      lT[k][j] = (gk < kend && gj < m) ? T[(long)gk * m + gj] : 0.0;
    }
    // stage trig panel: 32 freq-pairs x 16 toas, one sincos each
    for (int idx = tid; idx < 32 * 16; idx += 512) {
      const int p = idx / 16, k = idx % 16;
      const int gk = k0 + k;
      const int ceven = c0 + 2 * p;
      double sv = 0.0, cv = 0.0;
      if (gk < kend && ceven < F2) {
        const double wf = 2.0 * M_PI * freqs[ceven >> 1];
        sincos(wf * toas[gk], &sv, &cv);
        const double ni = ninv[gk];
        sv *= ni; cv *= ni;
      }
      lS[2 * p][k] = sv;
      lS[2 * p + 1][k] = cv;
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const double b = lS[jw + (lane & 15)][kk * 4 + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (rt_lo + q >= rt_hi) break;
        const double a =
            lT[kk * 4 + (lane >> 4)][rowbase + q * 16 + (lane & 15)];
        acc[q] = MFMA_F64(a, b, acc[q]);
      }
    }
    __syncthreads();
  }

  // epilogue: store (row j, col c) — cols contiguous, coalesced
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (rt_lo + q >= rt_hi) break;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = mbase + rowbase + q * 16 + 4 * v + (lane >> 4);
      const int col = c0 + jw + (lane & 15);
      if (col < F2) outp[(long)row * ldo + col] = acc[q][v];
    }
  }
}

// ---------------------------------------------------------------------
// chol_batch: per draw d, assemble Sigma = TNT + diag(phiinv[d]) (+
// identity padding to mp) in LDS, factor L L^T = Sigma (right-looking,
// NB=16 blocks, MFMA trailing updates), invert each 16x16 diagonal
// block, write L (D, mp, mp) and invdiag (D, mp/16, 16, 16).
// grid = (D, P), block = 256 (mp <= 64) or 512.  The 16x16 diagonal
// factor and its inversion run REGISTER-resident in wave 0 with DPP
// row broadcasts (row_bcast) -- the LDS read-modify-write chains of
// the naive version were the kernel's dominant cost
// (profiles/r01_initial_stats.md), and the LDS permutes of the __shfl
// version that followed it were a third of what remained.
// ---------------------------------------------------------------------
// (A (+i)-rotation column swizzle in place of the +1 row pad would
// shave Ash from 33.3 to 32.0 KB at mp=64 — one more workgroup per CU
// — but the extra address arithmetic measured +16 VGPR, dropping a
// waves/SIMD tier: net zero.  Padded layout kept.)
//
// Sigma is LOWER-TRIANGLE-packed — row i holds i+1 entries (+1 pad),
// halving LDS against a square layout (33.3 -> 17.4 KB at mp=64) so ~7
// workgroups fit per CU instead of 4, and at mp=128 two instead of one
// (the square layout is 132 KB); concurrency is the suspected chol
// bottleneck (82% parked waves resist every other explanation tested)
// and packing measured -13% on chol at the bench shape.  All
// factor-phase accesses are at-or-below the diagonal; the diagonal
// tile's upper half is read through the symmetric mirror AS_, and
// trailing stores into diagonal tiles are lower-guarded.
#define A_(i, j) Ash[(i) * ((i) + 3) / 2 + (j)]
#define AS_(i, j) ((j) <= (i) ? A_(i, j) : A_(j, i))

// (Forcing a 6-waves/SIMD allocation target on the small shapes got
// there only by spilling 44 B/lane and measured neutral — reverted;
// the no-spill allocation already reaches 5 waves.)

// Lane T of every 16-lane row, broadcast to that row: DPP row_newbcast
// (control 0x150 + T), a register move where a constant-lane
// __shfl(.., T, 16) is two LDS-permute round trips.  T must be a
// compile-time constant after unrolling, hence the switch.  A DPP read
// of a lane that EXEC masks off returns the bound-control zero, not the
// lane's value: call with all 64 lanes active.
static __device__ __forceinline__ double row_bcast(double w, int t) {
  int lo = __double2loint(w), hi = __double2hiint(w);
  switch (t) {
#define ROW_BCAST_CASE(T)                                                  \
    case T:                                                                \
      lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + T, 0xF, 0xF, true);  \
      hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + T, 0xF, 0xF, true);  \
      break;
    ROW_BCAST_CASE(0) ROW_BCAST_CASE(1) ROW_BCAST_CASE(2) ROW_BCAST_CASE(3)
    ROW_BCAST_CASE(4) ROW_BCAST_CASE(5) ROW_BCAST_CASE(6) ROW_BCAST_CASE(7)
    ROW_BCAST_CASE(8) ROW_BCAST_CASE(9) ROW_BCAST_CASE(10) ROW_BCAST_CASE(11)
    ROW_BCAST_CASE(12) ROW_BCAST_CASE(13) ROW_BCAST_CASE(14)
    ROW_BCAST_CASE(15)
#undef ROW_BCAST_CASE
  }
  return __hiloint2double(hi, lo);
}

// T0 (0, 4, 8 or 12): the first T0 rows and columns of Sigma are known
// to be an exact identity block (the leading pad of the stacked
// compressed system, T0 <= lead), and diagonal block 0 leaves out the
// steps that would factor and invert it.
template <int NBT, int T0 = 0>
__global__ __launch_bounds__(512, 4) void chol_batch_kernel(
    const double* __restrict__ TNT_all /*(P,m,m)*/,
    const double* __restrict__ phiinv_all /*(P,D,m)*/, int m, int D,
    double* __restrict__ L_all /*(P*D,mp,mp)*/,
    double* __restrict__ invd_all /*(P*D, mp/16, 16, 16)*/,
    // second diagonal source (phiinv_all null): the prior rows where
    // the phi assembly left them.  Entry (p, d, i) is at
    // rows_all[p * rows_ps + d * rows_ds + i]; the diagonal is 0 on the
    // `lead` leading identity rows of TNT and behind them, for i < m -
    // lead, rows[i] (delta0_all null) or 1 / (rows[i] - delta0[p][i])
    const double* __restrict__ rows_all, long rows_ps, long rows_ds,
    const double* __restrict__ delta0_all /*(P, m-lead)*/, int lead) {
  // grid.y batches PULSARS: one launch factors every (pulsar, draw)
  const int pp = blockIdx.y;
  const double* TNT = TNT_all + (long)pp * m * m;
  const double* phiinv = phiinv_all + (long)pp * D * m;
  const double* rows = rows_all + (long)pp * rows_ps;
  const double* delta0 = delta0_all + (long)pp * (m - lead);
  double* L = L_all + (long)pp * D * (NBT * 16) * (NBT * 16);
  double* invd = invd_all + (long)pp * D * NBT * 256;
  // LDS is sized by the template so small matrices keep multiple
  // workgroups per CU (nb=4: 33 KB -> 4 WG/CU vs one at 134 KB; the
  // serial diagonal phases then overlap ACROSS workgroups -- the PMC
  // profile showed 84% of wave cycles parked, profiles/).
  constexpr int mp = NBT * 16;
  __shared__ double Ash[mp * (mp + 3) / 2];
  __shared__ double inv16[2][16][17];

  const int d = blockIdx.x;
  if (d >= D) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  constexpr int nb = NBT;

  const int nthr = blockDim.x;
  const int nwv = nthr >> 6;
  // From the prior rows, the diagonal is the last mp threads', one entry
  // each: they load ahead of the assembly loop and divide behind it.
  // (The division inside the loop ran in every wave on every pass, a
  // diagonal entry being 65 apart: +8% on the isolated factor.)
  const bool inrows = phiinv_all == nullptr;
  const int di = inrows ? tid - (nthr - mp) : -1;
  double dtnt = 0.0, dsrc = 0.0, dsub = 0.0;
  if (di >= 0 && di < m) {
    dtnt = TNT[(long)di * m + di];
    if (di >= lead) {
      dsrc = rows[(long)d * rows_ds + (di - lead)];
      if (delta0_all != nullptr) dsub = delta0[di - lead];
    }
  }
  // assemble Sigma in LDS (lower triangle only)
  for (int idx = tid; idx < mp * mp; idx += nthr) {
    const int i = idx / mp, j = idx % mp;
    if (j > i) continue;
    double v = (i < m && j < m) ? TNT[(long)i * m + j] : 0.0;
    if (i == j) {
      if (inrows) continue;
      v += (i < m) ? phiinv[(long)d * m + i] : 1.0;
    }
    A_(i, j) = v;
  }
  if (di >= 0) {
    // SolveSystem.diag's operations in its order; the division is
    // correctly rounded, as torch's reciprocal is
    double dg = 1.0;  // the identity pad behind m
    if (di < lead)
      dg = 0.0;
    else if (di < m)
      dg = (delta0_all != nullptr) ? 1.0 / (dsrc - dsub) : dsrc;
    A_(di, di) = dtnt + dg;
  }
  __syncthreads();

  // Look-ahead right-looking Cholesky: the serial 16x16 diagonal
  // factor of column kb+1 (wave 0, register/DPP) runs CONCURRENTLY
  // with the MFMA trailing updates of columns kb+2.. (waves 1..7) --
  // the PMC profile showed 84-88% of wave cycles parked waiting on the
  // serial diagonal.  Two inverted-diagonal buffers ping-pong by kb
  // parity.
  //
  // The chain has no lane-dependent branch, so every row_bcast runs
  // with all 64 lanes active, and it issues a quarter fewer
  // instructions than one select per update.  At step t lane i updates
  // all of row[t+1..15], not only its lower-triangle entries j <= i.
  // An entry (i, j > i) then holds a value that means nothing, but it
  // only ever feeds entries (i, j' > j) of the same kind: a step reads
  // lane j's row[t] for t <= j alone, and only entries c <= i are
  // stored.  In the inversion x[t] is an exact +0.0 for t < c, so
  // fma(lrt, x[t], acc2) leaves acc2 (still +0.0 there) unchanged for
  // finite lrt and the t >= c select is not needed.  The entries that
  // are used see the same operations in the same order as under the
  // selects: L and invd keep every bit.
  //
  // TS > 0 (diagonal block 0 under T0): rows and columns < TS of the
  // block are an exact identity.  Steps t < TS of the factorisation are
  // sqrt(1), divisions by 1 and updates with an exact zero factor, rows
  // r < TS of the inversion are unit vectors and the terms t < TS of
  // the later rows multiply an exact zero of L: all left out.  Every
  // value keeps its bits except exact zeros of invd below the diagonal
  // in columns < TS, -0.0 from the full chain and +0.0 here.
#define CHOL_DIAG(KB, DST, TS)                                               \
  {                                                                          \
    const int dk0 = (KB)*NB;                                                 \
    const int i = lane & 15;                                                 \
    double row[16];                                                          \
    _Pragma("unroll") for (int c = 0; c < 16; ++c) row[c] =                  \
        AS_(dk0 + i, dk0 + c);                                               \
    _Pragma("unroll") for (int t = (TS); t < 16; ++t) {                      \
      const double dv = sqrt(row_bcast(row[t], t));                          \
      double rdv = 1.0 / dv;                                                 \
      /* every lane divides: a division kept to the lanes i != t is a  */   \
      /* branch, and the updates sink past it                          */   \
      asm volatile("" : "+v"(rdv));                                          \
      row[t] = (i == t) ? dv : row[t] * rdv;                                 \
      _Pragma("unroll") for (int j = t + 1; j < 16; ++j)                     \
        row[j] = fma(-row[t], row_bcast(row[t], j), row[j]);                 \
      /* one step at a time: hoisting later steps' broadcasts spills   */   \
      __builtin_amdgcn_sched_barrier(0);                                     \
    }                                                                        \
    _Pragma("unroll") for (int c = 0; c < 16; ++c) if (c <= i)               \
        A_(dk0 + i, dk0 + c) = row[c];                                       \
    const int c = i;                                                         \
    double x[16];                                                            \
    /* lane i computes only 1/L_ii; the rest arrive by broadcast (16x   */   \
    /* less serial f64 division work than every lane inverting all 16). */   \
    /* predicated select avoids a dynamic register index (scratch!)     */   \
    /* the reciprocal broadcast is inlined per r (a diag[16] register   */   \
    /* array cost ~16 VGPR and a waves/SIMD tier)                       */   \
    double dii = 0.0;                                                        \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) if (r == i) dii = row[r]; \
    const double myrcp = 1.0 / dii;                                          \
    _Pragma("unroll") for (int r = 0; r < (TS); ++r)                         \
        x[r] = (r == c) ? 1.0 : 0.0;                                         \
    _Pragma("unroll") for (int r = (TS); r < 16; ++r) {                      \
      const double dr = row_bcast(myrcp, r);                                 \
      double acc2 = 0.0;                                                     \
      _Pragma("unroll") for (int t = (TS); t < 16; ++t) {                    \
        const double lrt = row_bcast(row[t], r);                             \
        if (t < r) acc2 = fma(lrt, x[t], acc2);                              \
      }                                                                      \
      x[r] = (r < c) ? 0.0 : (r == c) ? dr : -acc2 * dr;                     \
      __builtin_amdgcn_sched_barrier(0);                                     \
    }                                                                        \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) (DST)[r][c] = x[r];       \
    if (lane < 16)                                                           \
      _Pragma("unroll") for (int r = 0; r < 16; ++r)                         \
          invd[((long)d * nb + (KB)) * 256 + r * 16 + c] = x[r];             \
  }

  // prologue: factor + invert diagonal block 0
  if (wv == 0) CHOL_DIAG(0, inv16[0], T0);
  __syncthreads();

  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * NB;

    // panel TRSM: row tiles below the diagonal, P <- P * inv(L_kk)^T
    for (int rt = kb + 1 + wv; rt < nb; rt += nwv) {
      const int r0 = rt * NB;
      f64x4 pacc = {0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double a = A_(r0 + (lane & 15), k0 + kk * 4 + (lane >> 4));
        const double b = inv16[kb & 1][lane & 15][kk * 4 + (lane >> 4)];
        pacc = MFMA_F64(a, b, pacc);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
        A_(r0 + 4 * v + (lane >> 4), k0 + (lane & 15)) = pacc[v];
    }
    __syncthreads();
    if (kb + 1 >= nb) break;

    // trailing phase A1: ONLY column kb+1 tiles, so its diagonal can
    // factor next (all waves)
    const int j1 = (kb + 1) * NB;
    for (int ib = kb + 1 + wv; ib < nb; ib += nwv) {
      const int i0 = ib * NB;
      f64x4 uacc;
      // diagonal tile (i0 == j1): upper half read via the symmetric
      // mirror, and its stores lower-guarded
#pragma unroll
      for (int v = 0; v < 4; ++v)
        uacc[v] = AS_(i0 + 4 * v + (lane >> 4), j1 + (lane & 15));
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double a = -A_(i0 + (lane & 15), k0 + kk * 4 + (lane >> 4));
        const double b = A_(j1 + (lane & 15), k0 + kk * 4 + (lane >> 4));
        uacc = MFMA_F64(a, b, uacc);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (i0 + 4 * v + (lane >> 4) >= j1 + (lane & 15))
          A_(i0 + 4 * v + (lane >> 4), j1 + (lane & 15)) = uacc[v];
    }
    __syncthreads();

    // phase A2: wave 0 factors diagonal kb+1 while the other waves do
    // the remaining trailing tiles (jb >= kb+2).  (Rotating the factor
    // wave across kb to spread the serial phase over SIMDs was
    // measured neutral with the LDS-permute chain and neutral to 1.5%
    // slower with the DPP chain — docs/TUNING_NOTES.md — and is not
    // built.)
    if (wv == 0) {
      CHOL_DIAG(kb + 1, inv16[(kb + 1) & 1], 0);
    } else {
      const int t = nb - kb - 2;
      const int ntile = t * (t + 1) / 2;
      for (int q = wv - 1; q < ntile; q += nwv - 1) {
        int ib = kb + 2, rem = q;
        while (rem > ib - kb - 2) { rem -= (ib - kb - 1); ++ib; }
        const int jb = kb + 2 + rem;
        const int i0 = ib * NB, j0 = jb * NB;
        f64x4 uacc;
#pragma unroll
        for (int v = 0; v < 4; ++v)
          uacc[v] = AS_(i0 + 4 * v + (lane >> 4), j0 + (lane & 15));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double a = -A_(i0 + (lane & 15), k0 + kk * 4 + (lane >> 4));
          const double b = A_(j0 + (lane & 15), k0 + kk * 4 + (lane >> 4));
          uacc = MFMA_F64(a, b, uacc);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (i0 + 4 * v + (lane >> 4) >= j0 + (lane & 15))
            A_(i0 + 4 * v + (lane >> 4), j0 + (lane & 15)) = uacc[v];
      }
    }
    __syncthreads();
  }
#undef CHOL_DIAG

  // write back L (full rows; the upper triangle is never read and
  // gets deterministic zeros)
  for (int idx = tid; idx < mp * mp; idx += nthr) {
    const int i = idx / mp, j = idx % mp;
    L[((long)d * mp + i) * mp + j] = (j > i) ? 0.0 : A_(i, j);
  }
}

// ---------------------------------------------------------------------
// trsm_fp: per (draw, frequency-tile) forward-substitute
//   W = L^-1 [B_cols | u]   (u = the T^T N^-1 r column, solved
//   redundantly per tile: one column vs 126)
// ENTIRELY IN REGISTERS, fused with the per-frequency reduction
//   M = sNs - [Ws.Ws, Ws.Wc; ., Wc.Wc],  N = sNr - [Ws.wu, Wc.wu]
//   Fp[d,f] += 0.5 * N^T M^-1 N   (closed-form 2x2)
//
// Key identity (probed layout, tools/mfma_probe.hip): the MFMA D/C
// accumulator layout of a 16x16 tile IS the B-fragment layout across
// k-steps -- value (row 4v+g, col j) lives in lane (g<<4)|j reg v, and
// the b-operand for k-step kk wants (row kk*4 + (l>>4), col l&15),
// i.e. reg kk of the SAME lane.  So the blocked forward substitution
// runs with W held in registers (acc layout), zero cross-lane moves:
//   acc  = -RHS_rb;  acc += sum_cb L[rb,cb] (x) W[cb]   (a from LDS Lp)
//   W[rb] = Iv[rb] (x) (-acc)                           (a from LDS Iv)
// The reduction is also register/shfl-resident (a frequency's sin/cos
// columns are ADJACENT lanes); LDS holds only the double-buffered L
// row-panel, the inverted diagonal blocks and the tiny solved-u column
// (~18 KB at the compressed shape -> 4 WG/CU, occupancy bounded by the
// 61-VGPR budget at 8 waves/SIMD).
// grid = (ceil(F/63), ceil(D/DPG), P);  block = 512 (8 waves)
// cols layout: [s0 c0 s1 c1 ... s62 c62 | u | pad]
// ---------------------------------------------------------------------
#define FPT_COLS 128
#define FPT_FREQS 63
#define NBMAX (FASTFP_MAXMP / 16)

// The 2x2 closure of one frequency: corrected products from the
// reduced dots, then Fp = 0.5 N^T M^-1 N in closed form.  One function
// for trsm_fp_kernel and trsm_fp_draws_kernel, so both emit the same
// operations and their results agree bit for bit.
static __device__ __forceinline__ double fp_close(
    double s11, double s22, double s12, double r1, double r2, double gsign,
    double ss, double cc, double sc, double su, double cu) {
  const double M11 = s11 - gsign * ss;
  const double M22 = s22 - gsign * cc;
  const double M12 = s12 - gsign * sc;
  const double N1 = r1 - gsign * su;
  const double N2 = r2 - gsign * cu;
  const double det = fma(M11, M22, -M12 * M12);
  const double num =
      fma(N1 * N1, M22, fma(-2.0 * N1, N2 * M12, N2 * N2 * M11));
  return 0.5 * num / det;
}

// PRODS: products mode for the sky-coherent Fe statistic — the
// epilogue stores the five corrected products [M11, M22, M12, N1, N2]
// = [s|s, c|c, s|c, s|r, c|r] un-collapsed into
// out[((p*D + d)*5 + i)*F + f] (plain stores, no accumulation) instead
// of reducing them to Fp.
template <int NBT, int DPG, bool PRODS = false>
__global__ __launch_bounds__(512, 4) void trsm_fp_kernel(
    const double* __restrict__ L_all /*(P*D,mp,mp)*/,
    const double* __restrict__ invd_all /*(P*D, mp/16, 16, 16)*/,
    const double* __restrict__ RHS_all /*(P, mp, 2F+1)*/,
    const double* __restrict__ sNs_all /*(P,3,F)*/,
    const double* __restrict__ sNr_all /*(P,2,F)*/, int F, int D,
    double gsign,
    double* __restrict__ fp_all /*(P,D,F); PRODS: (P,D,5,F)*/) {
  // grid.z batches PULSARS (one launch per draw chunk); each pulsar
  // accumulates into its own fp plane, summed deterministically by the
  // caller (no cross-pulsar races, no atomics).
  // gsign: +1 for the direct path (M = sNs - W.W), -1 for the
  // Schur-compressed draw path (M = M0 + W.W) -- docs/DESIGN.md.
  // NBT = mp/16 is a template parameter so every W[] index below is
  // compile-time: with a runtime index the register array is demoted to
  // scratch (288 B/lane measured) and every MFMA b-operand becomes a
  // memory load -- the whole point of the register-resident design.
  // DPG = draws per workgroup.  Only DPG=1 is instantiated: measured,
  // its 8 waves/SIMD at 61 VGPR beat DPG=2 (two draws sharing the Lp/Iv
  // staging and barriers, 4 waves/SIMD) by ~5%.  The body stays
  // written for a general DPG: with the draw count made a constant
  // (the ndr edge clamp below is a run-time value) the compiler emits
  // different instructions and register counts at every NBT, and the
  // code as generated today is the one that was measured.
  constexpr int mp = NBT * 16;
  __shared__ double Lp[2][DPG][16][NBT * 16 + 1];  // double-buffered
  __shared__ double Iv[DPG][NBT][16][17];
  __shared__ double Wu[DPG][NBT * 16];  // the solved u column

  const int pp = blockIdx.z;
  const double* L = L_all + (long)pp * D * mp * mp;
  const double* invd = invd_all + (long)pp * D * NBT * 256;
  const double* RHS = RHS_all + (long)pp * mp * (2L * F + 1);
  const double* sNs = sNs_all + (long)pp * 3 * F;
  const double* sNr = sNr_all + (long)pp * 2 * F;
  double* fp = fp_all + (long)pp * D * F;
  const int d0 = blockIdx.y * DPG;
  const int f0 = blockIdx.x * FPT_FREQS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const long ldr = 2L * F + 1;
  const int jw = wv * 16;      // this wave's 16-column strip
  const int li = lane & 15;    // a-frag row / strip column
  const int lk = lane >> 4;    // k index / acc row group
  const int ndr = min(DPG, D - d0);  // draws handled here (edge: D odd)

  // stage ALL inverted diagonal blocks once (both draws)
  for (int idx = tid; idx < ndr * NBT * 256; idx += 512) {
    const int e = idx / (NBT * 256);
    const int r = idx % (NBT * 256);
    Iv[e][r >> 8][(r >> 4) & 15][r & 15] =
        invd[((long)(d0 + e) * NBT) * 256 + r];
  }

  // load this wave's RHS strip into registers (acc layout):
  // W[e][rt][v] = RHS[row = rt*16 + 4v + lk][block-col jw + li]
  // (same RHS for every draw)
  const int bc = jw + li;
  f64x4 W[DPG][NBT];
#pragma unroll
  for (int rt = 0; rt < NBT; ++rt) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long row = rt * 16 + 4 * v + lk;
      double val = 0.0;
      if (bc < 126) {
        const long gc = 2L * f0 + bc;
        if (gc < 2L * F) val = RHS[row * ldr + gc];
      } else if (bc == 126) {
        val = RHS[row * ldr + 2L * F];  // the u column
      }
#pragma unroll
      for (int e = 0; e < DPG; ++e) W[e][rt][v] = val;
    }
  }
  __syncthreads();  // Iv staged

  // blocked forward substitution, W in registers, DPG draws
  // interleaved.  The L row-panel is DOUBLE-BUFFERED: each iteration
  // stages the NEXT row block's panel while computing on the current
  // one, so there is ONE barrier per row block instead of two and the
  // staging loads hide under the MFMA phase (the PMC profile charged
  // ~30% of wave cycles to the staging barriers).
#pragma unroll
  for (int rb = 0; rb < NBT; ++rb) {
    if (rb + 1 < NBT) {
      const int ncols = (rb + 1) * 16;
      for (int idx = tid; idx < ndr * 16 * ncols; idx += 512) {
        const int e = idx / (16 * ncols);
        const int q = idx % (16 * ncols);
        const int r = q / ncols, c = q % ncols;
        Lp[(rb + 1) & 1][e][r][c] =
            L[((long)(d0 + e) * mp + (rb + 1) * 16 + r) * mp + c];
      }
    }
    // two accumulator chains per draw (even/odd cb) deepen the MFMA
    // pipeline; folded together before the diagonal solve
    f64x4 acc[DPG], acc2[DPG];
#pragma unroll
    for (int e = 0; e < DPG; ++e) {
      acc[e] = -W[e][rb];  // -RHS_rb
      acc2[e] = f64x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int cb = 0; cb < rb; ++cb) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int e = 0; e < DPG; ++e) {
          const double a = Lp[rb & 1][e][li][cb * 16 + kk * 4 + lk];
          if (cb & 1)
            acc2[e] = MFMA_F64(a, W[e][cb][kk], acc2[e]);
          else
            acc[e] = MFMA_F64(a, W[e][cb][kk], acc[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < DPG; ++e) acc[e] += acc2[e];
    // W[rb] = Iv[rb] * (RHS - sum) = Iv[rb] * (-acc)
    // (a split even/odd-kk chain costs 7 extra VGPRs -> occupancy
    // 8 -> 7 waves/SIMD and measures SLOWER; keep the single chain)
    f64x4 sol[DPG];
#pragma unroll
    for (int e = 0; e < DPG; ++e) sol[e] = f64x4{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int e = 0; e < DPG; ++e) {
        const double a = Iv[e][rb][li][kk * 4 + lk];
        sol[e] = MFMA_F64(a, -acc[e][kk], sol[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < DPG; ++e) W[e][rb] = sol[e];
    __syncthreads();  // panel rb+1 staged for all; Lp[rb&1] reads done
  }

  // fused reduction, register-resident: a frequency's sin/cos columns
  // are ADJACENT lanes (li even/odd), so the per-frequency dots come
  // from __shfl_xor(w, 1) products accumulated in registers across
  // (rt, v); only the solved u column (wave 7, li == 14) goes through a
  // tiny LDS stage.  No barriers inside the accumulation loop (the
  // LDS-staged 16-row variant cost 2*NBT barriers per draw and
  // dominated the kernel at small NBT).
  if (wv == 7) {
#pragma unroll
    for (int rt = 0; rt < NBT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int e = 0; e < DPG; ++e)
          if (li == 14) Wu[e][rt * 16 + 4 * v + lk] = W[e][rt][v];
  }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < DPG; ++e) {
    if (e >= ndr) break;
    // lane-split accumulation: a frequency's sin column is an even
    // lane, its cos column the adjacent odd lane, and the quadratics
    // pair up — w*w accumulates ss on even lanes and cc on odd lanes
    // in the SAME register (likewise w*wu -> su/cu; w*wp is sc on
    // both).  3 fma chains instead of 5; the odd-lane halves arrive
    // by two shfl_xor after the row-group reduction.
    double a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int rt = 0; rt < NBT; ++rt) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const double w = W[e][rt][v];
        const double wp = __shfl_xor(w, 1, 64);  // partner column
        const double wu = Wu[e][rt * 16 + 4 * v + lk];
        a1 = fma(w, w, a1);
        a2 = fma(w, wu, a2);
        a3 = fma(w, wp, a3);
      }
    }
    // sum the 4 row groups (lanes lk = 0..3 share li): +16, +32 lanes
    a1 += __shfl_down(a1, 32, 64); a1 += __shfl_down(a1, 16, 64);
    a2 += __shfl_down(a2, 32, 64); a2 += __shfl_down(a2, 16, 64);
    a3 += __shfl_down(a3, 32, 64); a3 += __shfl_down(a3, 16, 64);
    const double b1 = __shfl_xor(a1, 1, 64);  // cc (for even lanes)
    const double b2 = __shfl_xor(a2, 1, 64);  // cu
    const int q = (jw + li) >> 1;  // frequency index within the block
    if (lk == 0 && (li & 1) == 0 && q < FPT_FREQS && f0 + q < F) {
      const int f = f0 + q;
      if constexpr (PRODS) {
        double* o = fp_all + (((long)pp * D + (d0 + e)) * 5) * F + f;
        o[0] = sNs[f] - gsign * a1;
        o[F] = sNs[F + f] - gsign * b1;
        o[2L * F] = sNs[2 * F + f] - gsign * a3;
        o[3L * F] = sNr[f] - gsign * a2;
        o[4L * F] = sNr[F + f] - gsign * b2;
      } else {
        fp[(long)(d0 + e) * F + f] +=
            fp_close(sNs[f], sNs[F + f], sNs[2 * F + f], sNr[f], sNr[F + f],
                     gsign, a1, b1, a3, a2, b2);
      }
    }
  }
}

// ---------------------------------------------------------------------
// trsm_fp_draws: the solve and reduction of trsm_fp_kernel<NBT,1> with
// the loop over DRAWS inside the workgroup.  A workgroup owns one
// (pulsar, frequency tile, draw slice [dlo, dhi)): its RHS strip (in
// registers) and its sNs/sNr entries (in LDS) are loaded ONCE and every
// draw of the slice is solved from them, so the per-draw traffic is the
// factor alone.  Draw d+1's factor goes from L and invd straight into
// the other LDS buffer by 16-byte direct loads (global_load_lds_dwordx4,
// no register in between) issued in front of draw d's MFMAs and waited
// for at draw d's barrier: one barrier per draw.  fp[p, d, f] is a plain
// store and is never read.  NBT 1..4 (mp <= 64).
//
// Same numbers as trsm_fp_kernel accumulating into zeros, bit for bit:
// the MFMA order per column, the acc/acc2 split, the order of every fma
// chain of the lane-split reduction and fp_close are its own.  Three
// things differ in form only:
//   * the strict-lower panels sit in LDS as the factor kernel wrote them
//     and their MFMAs negate the a operand (neg:[1,0,0], free and exact),
//     with acc starting at +RHS: acc holds the exact negative of
//     trsm_fp_kernel's (every fma of the chain is sign-symmetric) and the
//     diagonal solve takes it as it is — no negation of 8 + 8 registers
//     per row block per draw, and none of the staged panels either;
//   * the w*w and w*partner sums of row block rb are taken as soon as
//     W[rb] exists, in the shadow of the next row block's MFMAs; only
//     the w*u sum waits for the barrier that publishes the u column;
//   * the partner column (lane ^ 1) comes by DPP, not by an LDS permute.
//
// SKIP (0..3) is the caller's promise that the first 4*SKIP rows of the
// RHS are zero and that the system starts with an identity block of that
// size (L[4*SKIP:, :4*SKIP] = 0), as the engine's compressed stack pads
// m_v = 60 to 64 in FRONT.  W rows 0 .. 4*SKIP-1 are then exact zeros,
// and for kk < SKIP the kernel leaves out the MFMA of every cb = 0
// update and of row block 0's diagonal multiply: products with an exact
// zero operand, so no bit changes against SKIP = 0 on the same system.
// Every other MFMA and every fma keeps its order.  MFMAs per wave and
// draw at NBT = 4: 40, 36, 32, 28 for SKIP 0..3 (NBT fewer per step).
//
// Grid: 1-D, 8 * ceil(P*nsl / 8) * ntile blocks, decoded as
//   g = bid % 8, j = bid / 8, slice s = (j / ntile) * 8 + g,
//   tile = j % ntile, pulsar = s / nsl, draws [(s % nsl) * dpb, +dpb)
// so the ntile tiles of one (pulsar, slice) share bid % 8 — blocks that
// share an XCD's L2 — and are dispatched together: they walk the same
// draws and each factor comes from HBM about once.  Placement changes
// speed only.  Blocks with s >= P*nsl (grid padding) return at once.
//
// LDS (one array, 48.5 KiB at NBT=4):
//   2 buffers x (NBT(NBT-1)/2 strict-lower + NBT inverted-diagonal)
//     16x16 blocks, rows padded to 18 doubles: the a-fragment read
//     18*li + lk is conflict-free over a 32-lane half.  A buffer is
//     (NLB + NBT) * 144 16-byte pieces in lane-linear order, nine per
//     row, which is what a direct load writes (wave base + lane * 16);
//     the ninth piece of a row, the pad, is a second copy of the eighth;
//   2 x mp doubles: the solved u column, by draw parity;
//   5 x 64 doubles: sNs/sNr of the tile's frequencies.
// block = 512 (8 waves), tile = 63 frequencies + u as in trsm_fp_kernel.
// Registers as compiled (gfx950, -O3), SKIP = 0 / 1 / 2 / 3: NBT=4
// 106 / 104 / 98 / 96 VGPR, 4 waves/SIMD (two workgroups per CU), NBT=3
// 79 / 77 / 82 / 72, NBT=2 61 / 59 / 57 / 55, NBT=1 42 / 40 / 38 / 36;
// no scratch anywhere.  RHS copy 8*NBT, W 8*NBT, the three accumulators
// 24, the source pointers and strides of the direct loads
// 3 * ceil((NLB + NBT) * 144 / 512).  LDS is the same for every SKIP.
//
// PRODS: products mode (Fe), as trsm_fp_kernel's — the closing lane
// stores the five corrected products into out[((p*D + d)*5 + i)*F + f]
// (plain vector stores, every entry written, none read) instead of
// closing them to Fp.  Solve, staging and the three sums are shared, so
// the values equal trsm_fp_kernel<NBT, 1, true>'s bit for bit at every
// SKIP.  As compiled, all 16 PRODS instantiations have the VGPR and
// SGPR counts and the LDS of the Fp instantiation with the same NBT and
// SKIP in the table above (SGPRs 42 / 44 / 42 / 42 at NBT 1..4, 40 at
// NBT=1 SKIP=3).
// ---------------------------------------------------------------------
#define DL_BS 18              // row stride of a staged block (doubles)
#define DL_BLK (16 * DL_BS)   // doubles per staged block
#define DL_FREQS 63           // frequencies per tile

// the value of lane ^ 1 (a frequency's partner column) by DPP
// quad_perm [1,0,3,2]: a register move, no LDS permute traffic.  Call
// with all lanes active.
static __device__ __forceinline__ double pair_swap(double w) {
  int lo = __double2loint(w), hi = __double2hiint(w);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <int NBT, int SKIP, bool PRODS = false>
__global__ __launch_bounds__(512, 4) void trsm_fp_draws_kernel(
    const double* __restrict__ L_all /*(P*D,mp,mp)*/,
    const double* __restrict__ invd_all /*(P*D, mp/16, 16, 16)*/,
    const double* __restrict__ RHS_all /*(P, mp, 2F+1)*/,
    const double* __restrict__ sNs_all /*(P,3,F)*/,
    const double* __restrict__ sNr_all /*(P,2,F)*/, int F, int D, int P,
    int dpb /*draws per block*/, int nsl /*slices = ceil(D/dpb)*/,
    double gsign,
    double* __restrict__ fp_all /*(P,D,F); PRODS: (P,D,5,F)*/) {
  constexpr int mp = NBT * 16;
  constexpr int UC = 126;  // block column of u
  constexpr int NLB = NBT * (NBT - 1) / 2;  // strict-lower blocks
  constexpr int BUF = (NLB + NBT) * DL_BLK;
  __shared__ __attribute__((aligned(16))) double S[2 * BUF + 2 * mp + 5 * 64];

  const int ntile = (F + DL_FREQS - 1) / DL_FREQS;
  const int j = blockIdx.x >> 3;
  const int s = (j / ntile) * 8 + (blockIdx.x & 7);
  if (s >= P * nsl) return;
  const int pp = s / nsl;
  const int dlo = (s % nsl) * dpb;
  const int dhi = min(D, dlo + dpb);
  const int f0 = (j % ntile) * DL_FREQS;

  const double* L = L_all + (long)pp * D * mp * mp;
  const double* invd = invd_all + (long)pp * D * NBT * 256;
  const double* RHS = RHS_all + (long)pp * mp * (2L * F + 1);
  const double* sNs = sNs_all + (long)pp * 3 * F;
  const double* sNr = sNr_all + (long)pp * 2 * F;
  double* fp = fp_all + (long)pp * D * F;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const long ldr = 2L * F + 1;
  const int jw = wv * 16;      // this wave's 16-column strip
  const int li = lane & 15;    // a-frag row / strip column
  const int lk = lane >> 4;    // k index / acc row group

  // factor of the next draw -> LDS buffer `buf` by 16-byte direct loads
  // (no register in between).  The staged image is NP 16-byte pieces,
  // nine per 18-double row; piece p of it comes from block p / 144, row
  // (p % 144) / 9, and the ninth piece of a row — the two pad doubles no
  // a-fragment reads — re-reads the row's eighth, so every source is
  // inside L or invd.  A thread owns pieces tid + 512 i: their sources
  // are found once per slice and advance by one draw per call.  The
  // destination of a wave's load is its base + lane * 16, which is the
  // image's own order.
  constexpr int NP = (NLB + NBT) * (DL_BLK / 2);
  constexpr int NPT = (NP + 511) / 512;  // pieces per thread
  const double* src[NPT];
  int inc[NPT];  // doubles from one draw's piece to the next draw's
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int p = min(tid + 512 * i, NP - 1);
    const int blk = p / (DL_BLK / 2), r = (p % (DL_BLK / 2)) / 9;
    const int c = 2 * min(p % 9, 7);
    if (blk < NLB) {  // strict-lower block rb(rb-1)/2 + cb of L
      const int rb = 1 + (blk >= 1) + (blk >= 3);
      const int cb = blk - rb * (rb - 1) / 2;
      src[i] = L + (long)dlo * mp * mp + (rb * 16 + r) * mp + cb * 16 + c;
      inc[i] = mp * mp;
    } else {  // inverted diagonal block blk - NLB
      src[i] = invd + (long)dlo * NBT * 256 + (blk - NLB) * 256 + r * 16 + c;
      inc[i] = NBT * 256;
    }
  }
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  auto dma = [&](double* buf) {
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      if (512 * (i + 1) <= NP || tid + 512 * i < NP)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)src[i],
            (__attribute__((address_space(3))) void*)(buf +
                                                      2 * (512 * i + 64 * wvu)),
            16, 0, 0);
      src[i] += inc[i];
    }
  };

  dma(S);

  // this wave's RHS strip, acc layout, kept for the whole slice:
  // R0[rt][v] = RHS[row = rt*16 + 4v + lk][block-col jw + li]
  const int bc = jw + li;
  f64x4 R0[NBT];
#pragma unroll
  for (int rt = 0; rt < NBT; ++rt) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long row = rt * 16 + 4 * v + lk;
      double val = 0.0;
      if (bc < UC) {
        const long gc = 2L * f0 + bc;
        if (gc < 2L * F) val = RHS[row * ldr + gc];
      } else if (bc == UC) {
        val = RHS[row * ldr + 2L * F];  // the u column
      }
      R0[rt][v] = val;
    }
  }
  // the tile's sNs/sNr entries: Sc[i][q], q = frequency within the tile
  double* Sc = S + 2 * BUF + 2 * mp;
  if (tid < 64) {
    const bool live = tid < DL_FREQS && f0 + tid < F;
    const int fq = live ? f0 + tid : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      Sc[i * 64 + tid] = live ? sNs[i * F + fq] : 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      Sc[(3 + i) * 64 + tid] = live ? sNr[i * F + fq] : 0.0;
  }
  const int q = bc >> 1;  // frequency index within the tile
  const int f = f0 + q;
  // the lane that closes frequency q
  const bool closer = lk == 0 && (li & 1) == 0 && q < DL_FREQS && f < F;

  __syncthreads();  // waits for the direct loads of draw dlo

  const int aoff = li * DL_BS + lk;  // a-fragment offset inside a block
  for (int d = dlo; d < dhi; ++d) {
    const int b = (d - dlo) & 1;
    const double* Sb = S + b * BUF;
    double* Wu = S + 2 * BUF + b * mp;
    // every wave is past the barrier that ended the reads of buffer
    // b ^ 1; the loads are waited for in front of this draw's barrier
    if (d + 1 < dhi) dma(S + (b ^ 1) * BUF);

    // blocked forward substitution from the register RHS copy; acc is
    // the negative of trsm_fp_kernel's (the MFMA negates the panels)
    f64x4 W[NBT];
    double a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int rb = 0; rb < NBT; ++rb) {
      f64x4 acc = R0[rb];
      f64x4 acc2 = f64x4{0, 0, 0, 0};
#pragma unroll
      for (int cb = 0; cb < rb; ++cb) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          if (cb == 0 && kk < SKIP) continue;  // W rows 4kk..4kk+3 are 0
          const double a =
              Sb[(rb * (rb - 1) / 2 + cb) * DL_BLK + kk * 4 + aoff];
          if (cb & 1)
            acc2 = MFMA_F64_NEGA(a, W[cb][kk], acc2);
          else
            acc = MFMA_F64_NEGA(a, W[cb][kk], acc);
        }
      }
      acc += acc2;
      f64x4 sol = f64x4{0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (rb == 0 && kk < SKIP) continue;  // acc rows 4kk..4kk+3 are 0
        const double a = Sb[(NLB + rb) * DL_BLK + kk * 4 + aoff];
        sol = MFMA_F64(a, acc[kk], sol);
      }
      W[rb] = sol;
      // lane-split sums that need no u column (see trsm_fp_kernel)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const double w = sol[v];
        const double wp = pair_swap(w);  // partner column
        a1 = fma(w, w, a1);
        a3 = fma(w, wp, a3);
      }
      // pin the partial sums here: left alone the scheduler sinks all
      // of them below the barrier and spills the partner values
      asm volatile("" : "+v"(a1), "+v"(a3));
    }
    if (wv == 7 && li == 14) {
#pragma unroll
      for (int rt = 0; rt < NBT; ++rt)
#pragma unroll
        for (int v = 0; v < 4; ++v) Wu[rt * 16 + 4 * v + lk] = W[rt][v];
    }
    // factor d+1 and u column d visible; every read of buffer b done
    __syncthreads();

#pragma unroll
    for (int rt = 0; rt < NBT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        a2 = fma(W[rt][v], Wu[rt * 16 + 4 * v + lk], a2);
    // sum the 4 row groups (lanes lk = 0..3 share li): +16, +32 lanes
    a1 += __shfl_down(a1, 32, 64); a1 += __shfl_down(a1, 16, 64);
    a2 += __shfl_down(a2, 32, 64); a2 += __shfl_down(a2, 16, 64);
    a3 += __shfl_down(a3, 32, 64); a3 += __shfl_down(a3, 16, 64);
    const double b1 = pair_swap(a1);  // cc (for even lanes)
    const double b2 = pair_swap(a2);  // cu
    if constexpr (PRODS) {
      // the five corrected products of trsm_fp_kernel<.., true>, same
      // expressions in the same order
      if (closer) {
        double* o = fp_all + (((long)pp * D + d) * 5) * F + f;
        o[0] = Sc[q] - gsign * a1;
        o[F] = Sc[64 + q] - gsign * b1;
        o[2L * F] = Sc[128 + q] - gsign * a3;
        o[3L * F] = Sc[192 + q] - gsign * a2;
        o[4L * F] = Sc[256 + q] - gsign * b2;
      }
    } else {
      if (closer)
        fp[(long)d * F + f] =
            fp_close(Sc[q], Sc[64 + q], Sc[128 + q], Sc[192 + q], Sc[256 + q],
                     gsign, a1, b1, a3, a2, b2);
    }
  }
}

// ---------------------------------------------------------------------
// trsm_fp_rl: RIGHT-LOOKING variant of trsm_fp.  The left-looking form
// accumulates each row block's correction in one (two, even/odd-split)
// dependent MFMA chain; at 64-cycle f64 MFMA dependent latency that
// caps the pipe near 55% (docs/TUNING_NOTES.md).  Right-looking
// applies each solved block's update to ALL remaining row blocks
// immediately:
//   solve  W[cb] = Iv[cb] (x) W[cb]          (4-MFMA chain)
//   update W[rb] -= L[rb][cb] (x) W[cb]      (independent chains, one
//                                             per remaining row block)
// Same MFMA count, same register state (W only — the separate acc
// chains vanish, saving 8 VGPRs), but most MFMAs now sit on
// independent accumulators, so the pipe can fill while the critical
// solve chain waits.  L is staged as COLUMN panels (double-buffered,
// row stride 19: conflict-free for the a-fragment access pattern
// 19*li + 4*kk + lk mod 32 banks).  Measured within +-2% of the
// left-looking kernel at NBT <= 8, so it is dispatched only for
// NBT 9..16 (128 < mp <= 256), where the left-looking kernel's extra
// accumulator chains would not fit the register budget.
// ---------------------------------------------------------------------
template <int NBT>
__global__ __launch_bounds__(512, 4) void trsm_fp_rl_kernel(
    const double* __restrict__ L_all /*(P*D,mp,mp)*/,
    const double* __restrict__ invd_all /*(P*D, mp/16, 16, 16)*/,
    const double* __restrict__ RHS_all /*(P, mp, 2F+1)*/,
    const double* __restrict__ sNs_all /*(P,3,F)*/,
    const double* __restrict__ sNr_all /*(P,2,F)*/, int F, int D,
    double gsign, double* __restrict__ fp_all /*(P,D,F)*/) {
  constexpr int mp = NBT * 16;
  constexpr int PROWS = NBT > 1 ? (NBT - 1) * 16 : 1;
  __shared__ double Lc[2][PROWS][19];  // column panel, double-buffered
  __shared__ double Iv[NBT][16][19];
  __shared__ double Wu[NBT * 16];  // the solved u column

  const int pp = blockIdx.z;
  const double* L = L_all + (long)pp * D * mp * mp;
  const double* invd = invd_all + (long)pp * D * NBT * 256;
  const double* RHS = RHS_all + (long)pp * mp * (2L * F + 1);
  const double* sNs = sNs_all + (long)pp * 3 * F;
  const double* sNr = sNr_all + (long)pp * 2 * F;
  double* fp = fp_all + (long)pp * D * F;
  const int d0 = blockIdx.y;
  const int f0 = blockIdx.x * FPT_FREQS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const long ldr = 2L * F + 1;
  const int jw = wv * 16;
  const int li = lane & 15;
  const int lk = lane >> 4;

  // stage inverted diagonal blocks
  for (int idx = tid; idx < NBT * 256; idx += 512)
    Iv[idx >> 8][(idx >> 4) & 15][idx & 15] =
        invd[(long)d0 * NBT * 256 + idx];

  // load RHS strip into registers (acc layout)
  const int bc = jw + li;
  f64x4 W[NBT];
#pragma unroll
  for (int rt = 0; rt < NBT; ++rt) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long row = rt * 16 + 4 * v + lk;
      double val = 0.0;
      if (bc < 126) {
        const long gc = 2L * f0 + bc;
        if (gc < 2L * F) val = RHS[row * ldr + gc];
      } else if (bc == 126) {
        val = RHS[row * ldr + 2L * F];  // the u column
      }
      W[rt][v] = val;
    }
  }

  // stage column panel 0 (rows 16..mp of column block 0)
  if (NBT > 1) {
    for (int idx = tid; idx < (NBT - 1) * 16 * 16; idx += 512) {
      const int r = idx >> 4, c = idx & 15;
      Lc[0][r][c] = L[((long)d0 * mp + 16 + r) * mp + c];
    }
  }
  __syncthreads();

#pragma unroll
  for (int cb = 0; cb < NBT; ++cb) {
    // solve W[cb] = Iv[cb] (x) W[cb]
    f64x4 sol = f64x4{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const double a = Iv[cb][li][kk * 4 + lk];
      sol = MFMA_F64(a, W[cb][kk], sol);
    }
    W[cb] = sol;
    // independent-accumulator updates of every remaining row block
#pragma unroll
    for (int rb = cb + 1; rb < NBT; ++rb) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double a = -Lc[cb & 1][(rb - cb - 1) * 16 + li][kk * 4 + lk];
        W[rb] = MFMA_F64(a, sol[kk], W[rb]);
      }
    }
    // prefetch the NEXT column panel (issued after the updates so its
    // address arithmetic doesn't inflate the MFMA region's live
    // registers; the loads still overlap the updates' latency since
    // nothing waits on them until the barrier)
    if (cb + 1 < NBT) {
      const int nrows2 = (NBT - 2 - cb) * 16;  // rows (cb+2)*16..mp
      for (int idx = tid; idx < nrows2 * 16; idx += 512) {
        const int r = idx >> 4, c = idx & 15;
        Lc[(cb + 1) & 1][r][c] =
            L[((long)d0 * mp + (cb + 2) * 16 + r) * mp + (cb + 1) * 16 + c];
      }
    }
    __syncthreads();
  }

  // fused register/shfl reduction — identical to trsm_fp_kernel
  if (wv == 7) {
#pragma unroll
    for (int rt = 0; rt < NBT; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (li == 14) Wu[rt * 16 + 4 * v + lk] = W[rt][v];
  }
  __syncthreads();

  // lane-split accumulation (see trsm_fp_kernel): 3 fma chains, odd
  // halves fetched by shfl_xor after the row-group reduction
  double a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
  for (int rt = 0; rt < NBT; ++rt) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const double w = W[rt][v];
      const double wp = __shfl_xor(w, 1, 64);
      const double wu = Wu[rt * 16 + 4 * v + lk];
      a1 = fma(w, w, a1);
      a2 = fma(w, wu, a2);
      a3 = fma(w, wp, a3);
    }
  }
  a1 += __shfl_down(a1, 32, 64); a1 += __shfl_down(a1, 16, 64);
  a2 += __shfl_down(a2, 32, 64); a2 += __shfl_down(a2, 16, 64);
  a3 += __shfl_down(a3, 32, 64); a3 += __shfl_down(a3, 16, 64);
  const double b1 = __shfl_xor(a1, 1, 64);
  const double b2 = __shfl_xor(a2, 1, 64);
  const int q = (jw + li) >> 1;
  if (lk == 0 && (li & 1) == 0 && q < FPT_FREQS && f0 + q < F) {
    const int f = f0 + q;
    const double M11 = sNs[f] - gsign * a1;
    const double M22 = sNs[F + f] - gsign * b1;
    const double M12 = sNs[2 * F + f] - gsign * a3;
    const double N1 = sNr[f] - gsign * a2;
    const double N2 = sNr[F + f] - gsign * b2;
    const double det = fma(M11, M22, -M12 * M12);
    const double num =
        fma(N1 * N1, M22, fma(-2.0 * N1, N2 * M12, N2 * N2 * M11));
    fp[(long)d0 * F + f] += 0.5 * num / det;
  }
}

// ---------------------------------------------------------------------
// diag_inv: invert the 16x16 diagonal blocks of a batch of lower-
// triangular L (B, mp, mp) -> invd (B, mp/16, 16, 16).  Used by the
// m > 128 direct path, where L comes from batched rocSOLVER Cholesky
// (the LDS-resident chol_batch kernel caps at mp = 128: Sigma no
// longer fits LDS above that).  One wave per (batch, block); register
// rows + width-16 shfl — same technique as chol_batch's CHOL_DIAG.
// grid.x = ceil(B * mp/16 / 8), block = 512 (8 waves)
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(512, 4) void diag_inv_kernel(
    const double* __restrict__ L, int mp, long nblk_total,
    double* __restrict__ invd) {
  const long w = (long)blockIdx.x * 8 + (threadIdx.x >> 6);
  if (w >= nblk_total) return;
  const int nbt = mp >> 4;
  const long b = w / nbt;
  const int kb = (int)(w % nbt);
  const int lane = threadIdx.x & 63;
  const int i = lane & 15;  // row; the 4 sub-groups compute redundantly
  const double* Lb = L + b * (long)mp * mp + (long)kb * 16 * mp + kb * 16;
  double row[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) row[c] = (c <= i) ? Lb[(long)i * mp + c] : 0.0;
  const int c = i;  // lane owns output column c
  double x[16];
  double dii = 1.0;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == i) dii = row[r];
  const double myrcp = 1.0 / dii;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const double dr = __shfl(myrcp, r, 16);
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double lrt = __shfl(row[t], r, 16);
      if (t >= c && t < r) acc = fma(lrt, x[t], acc);
    }
    x[r] = (r < c) ? 0.0 : (r == c) ? dr : -acc * dr;
  }
  if (lane < 16)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      invd[(b * nbt + kb) * 256 + r * 16 + c] = x[r];
}

// ---------------------------------------------------------------------
// Block-diagonal white noise (EcorrKernelNoise, BASELINE config 4):
// N is block-diagonal per observing epoch.  The reference never
// implemented this case (/root/reference/fastfp/utils.py:30-31,
// README.md:22).  Blocks are contiguous after the BlockNoise TOA
// permutation (fastfp_amd/blocknoise.py).
//
// Each block is diag(nvec) + e2*J (diagonal + rank-1), so the inverse
// is the Sherman-Morrison closed form
//   N_b^{-1} = D^{-1} - beta_b d d^T,  d = D^{-1} 1,
//   beta_b = e2 / (1 + e2 * sum(1/nvec_b))
// — no factorization, O(sz) per block, ANY epoch size (the round-1
// per-block Cholesky kernel and its 32-TOA cap are gone).
// ---------------------------------------------------------------------

// sigdots_block: the five per-frequency dots with BLOCK-diagonal N.
// sr/cr use the precomputed nr = N^{-1} r vector (host S-M solve); the
// quadratics are the diagonal part (uvec-weighted, like sigdots) minus
// the per-block rank-1 corrections beta_b * (d.s)_b (d.c)_b.
// grid.x = F, block = 256.
extern "C" __global__ __launch_bounds__(256) void sigdots_block_kernel(
    const double* __restrict__ toas, const double* __restrict__ uvec,
    const double* __restrict__ nr, const double* __restrict__ freqs,
    const double* __restrict__ beta, const long* __restrict__ offsets,
    const long* __restrict__ sizes, int nblk, int ntoa, int F,
    double* __restrict__ sNs, double* __restrict__ sNr) {
  const int f = blockIdx.x;
  if (f >= F) return;
  const double w = 2.0 * M_PI * freqs[f];
  double ss = 0, cc = 0, sc = 0, sr = 0, cr = 0;
  // diagonal part + the N^-1 r dots
  for (int i = threadIdx.x; i < ntoa; i += blockDim.x) {
    double s, c;
    sincos(w * toas[i], &s, &c);
    const double ui = uvec[i];
    const double ri = nr[i];
    ss = fma(s * s, ui, ss);
    cc = fma(c * c, ui, cc);
    sc = fma(s * c, ui, sc);
    sr = fma(s, ri, sr);
    cr = fma(c, ri, cr);
  }
  // rank-1 corrections: one weighted sum per block (any size)
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
    const double bb = beta[b];
    if (bb == 0.0) continue;  // singleton / no-ecorr block
    const long o = offsets[b];
    const int sz = (int)sizes[b];
    double us = 0.0, uc = 0.0;
    for (int i = 0; i < sz; ++i) {
      double s, c;
      sincos(w * toas[o + i], &s, &c);
      const double ui = uvec[o + i];
      us = fma(s, ui, us);
      uc = fma(c, ui, uc);
    }
    ss = fma(-bb * us, us, ss);
    cc = fma(-bb * uc, uc, cc);
    sc = fma(-bb * us, uc, sc);
  }
  __shared__ double red[4][5];
  ss = wave_reduce_sum(ss);
  cc = wave_reduce_sum(cc);
  sc = wave_reduce_sum(sc);
  sr = wave_reduce_sum(sr);
  cr = wave_reduce_sum(cr);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[wv][0] = ss; red[wv][1] = cc; red[wv][2] = sc;
    red[wv][3] = sr; red[wv][4] = cr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int v = 0; v < 4; ++v) {
      a0 += red[v][0]; a1 += red[v][1]; a2 += red[v][2];
      a3 += red[v][3]; a4 += red[v][4];
    }
    sNs[f] = a0; sNs[F + f] = a1; sNs[2 * F + f] = a2;
    sNr[f] = a3; sNr[F + f] = a4;
  }
}

// Plan and launch the draw-looping solve (mp <= 64) in either mode:
// PRODS = false stores Fp into out (P,D,F), PRODS = true the five
// products into out (P,D,5,F).  draws_per_block > 0 forces the slice
// length (tests); 0 sizes it from the resident workgroup slots
// (occupancy query x ncu): 64 draws where the launch allows — the
// one-time RHS load is then under 2% of a slice's traffic — and fewer
// when that would leave the launch under 8 rounds of resident blocks, so
// the partial last round stays a small fraction; slices are then evened
// out over D.
template <bool PRODS>
static int launch_draws(const double* L, const double* invd,
                        const double* RHS, const double* sNs,
                        const double* sNr, int mp, int F, int D, int P,
                        double gsign, double* out, int draws_per_block,
                        int ncu, int lead, hipStream_t stream) {
  if (lead < 0 || lead > 12 || (lead & 3)) return (int)hipErrorInvalidValue;
  const int ntile = (F + DL_FREQS - 1) / DL_FREQS;
  int dpb = draws_per_block, nsl = 0;
  auto plan = [&](auto kern) -> long {
    if (dpb <= 0) {
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 512,
                                                       0) != hipSuccess ||
          per_cu < 1)
        per_cu = 1;
      const long slots = (long)per_cu * ncu;
      const long units = (long)P * ntile * D;  // (tile, draw) pairs
      dpb = (int)std::min<long>(64, std::max<long>(1, units / (8 * slots)));
      dpb = std::min(dpb, D);
      const int n = (D + dpb - 1) / dpb;
      dpb = (D + n - 1) / n;
    }
    dpb = std::min(dpb, D);
    nsl = (D + dpb - 1) / dpb;
    return ((long)P * nsl + 7) / 8 * 8 * ntile;
  };
  if (mp < 16 || mp > 64 || (mp & 15)) return (int)hipErrorInvalidValue;
  switch ((mp >> 4) * 4 + (lead >> 2)) {
#define DRAWS_CASE(NBT, SKIP) \
    case NBT * 4 + SKIP: { \
      auto kern = trsm_fp_draws_kernel<NBT, SKIP, PRODS>; \
      const long nblk = plan(kern); \
      if (nblk >= (1L << 31)) return (int)hipErrorInvalidValue; \
      hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(512), 0, stream, \
                         L, invd, RHS, sNs, sNr, F, D, P, dpb, nsl, gsign, \
                         out); \
    } break;
#define DRAWS_NBT(NBT) \
    DRAWS_CASE(NBT, 0) DRAWS_CASE(NBT, 1) DRAWS_CASE(NBT, 2) DRAWS_CASE(NBT, 3)
    DRAWS_NBT(1) DRAWS_NBT(2) DRAWS_NBT(3) DRAWS_NBT(4)
#undef DRAWS_NBT
#undef DRAWS_CASE
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// Launch the one-draw-per-workgroup solve over (ftiles, D, P) in either
// mode.  PRODS = false accumulates Fp into out (P,D,F) and covers
// mp <= 256; PRODS = true stores the five products into out (P,D,5,F)
// and has mp <= 128 only.
template <bool PRODS>
static int launch_one_draw(const double* L, const double* invd,
                           const double* RHS, const double* sNs,
                           const double* sNr, int mp, int F, int D, int P,
                           double gsign, double* out, hipStream_t stream) {
  const int ftiles = (F + FPT_FREQS - 1) / FPT_FREQS;
  const dim3 grid(ftiles, D, P), blk(512);
  // the right-looking kernel below has no products mode
  if (PRODS && mp > FASTFP_MAXMP) return (int)hipErrorInvalidValue;
  switch (mp >> 4) {
#define TRSM_CASE(NBT) \
    case NBT: hipLaunchKernelGGL((trsm_fp_kernel<NBT, 1, PRODS>), grid, blk, \
                  0, stream, L, invd, RHS, sNs, sNr, F, D, gsign, out); break;
    TRSM_CASE(1) TRSM_CASE(2) TRSM_CASE(3) TRSM_CASE(4)
    TRSM_CASE(5) TRSM_CASE(6) TRSM_CASE(7) TRSM_CASE(8)
#undef TRSM_CASE
    // m > 128 (GP-ECORR direct path) dispatches the RIGHT-LOOKING
    // variant: its single in-place accumulator set (no acc/acc2
    // chains) keeps W = NBT*4 f64 regs per lane within budget at
    // NBT up to 16.  The FACTOR for these sizes comes from rocSOLVER
    // (chol_batch's LDS-resident Sigma caps at 128) + diag_inv.
#define TRSM_BIG_CASE(NBT) \
    case NBT: hipLaunchKernelGGL((trsm_fp_rl_kernel<NBT>), grid, blk, 0, \
                  stream, L, invd, RHS, sNs, sNr, F, D, gsign, out); break;
    TRSM_BIG_CASE(9) TRSM_BIG_CASE(10) TRSM_BIG_CASE(11) TRSM_BIG_CASE(12)
    TRSM_BIG_CASE(13) TRSM_BIG_CASE(14) TRSM_BIG_CASE(15) TRSM_BIG_CASE(16)
#undef TRSM_BIG_CASE
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------
// phi_inv_batch: the homogeneous prior phi^-1 of noise.batch_phiinv in
// one pass — out (P, D, ntm + nf), every entry written:
//   out[p, d, :ntm]     = tm_inv
//   out[p, d, ntm + k]  = 1 / (phi_rn[p, d, k] (+ phi_c[d, k], k < nc))
//   phi = f_k^-gam * (10^lgA)^2 * (1/12) * (1/pi^2) * fyr^(gam-3) * dff_k
// with the products in exactly this order and one rounding each (no
// FMA contraction), the operations of the torch chain the kernel
// replaces, so the result matches it bit for bit wherever the device
// pow is torch's.  A workgroup takes PHI_ROWS consecutive (p, d) rows:
// it first computes the per-row factors (10^lgA)^2 and fyr^(gam-3) of
// the red noise and of the common process once into LDS, then walks the
// rows' entries, a sine/cosine pair per thread — the two bins share
// their frequency, so one pow serves both.
// ---------------------------------------------------------------------
#define PHI_ROWS 16

extern "C" __global__ __launch_bounds__(256) void phi_inv_batch_kernel(
    const double* __restrict__ gam /*(P*D)*/,
    const double* __restrict__ lgA /*(P*D)*/,
    const double* __restrict__ gam_c /*(D) at stride c_dstride; nc > 0*/,
    const double* __restrict__ lgA_c, int c_dstride,
    const double* __restrict__ Ff /*(nf)*/,
    const double* __restrict__ dff /*(nf)*/,
    const double* __restrict__ Ff_c /*(nc)*/,
    const double* __restrict__ dff_c /*(nc)*/, int nf, int nc, int ntm,
    long nrows, int D, double ten, double fyr, double inv12, double invpi2,
    double tm_inv, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_ng[2][PHI_ROWS], s_a2[2][PHI_ROWS], s_fy[2][PHI_ROWS];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * PHI_ROWS;
  const int nr = (int)min((long)PHI_ROWS, nrows - r0);

  // per-row factors: threads [0, PHI_ROWS) the red noise of row r0 +
  // tid, threads [PHI_ROWS, 2 PHI_ROWS) the common process of its draw
  if (tid < 2 * PHI_ROWS) {
    const int which = tid / PHI_ROWS, rl = tid % PHI_ROWS;
    if (rl < nr && (which == 0 || nc > 0)) {
      const long r = r0 + rl;
      const long ci = (r % D) * c_dstride;
      const double g = which ? gam_c[ci] : gam[r];
      const double la = which ? lgA_c[ci] : lgA[r];
      const double a = pow(ten, la);
      s_ng[which][rl] = -g;
      s_a2[which][rl] = a * a;
      s_fy[which][rl] = pow(fyr, g - 3.0);
    }
  }
  __syncthreads();

  const int m = ntm + nf;
  const int w = ntm + nf / 2;  // entries of a row: tm bins, then pairs
  for (int idx = tid; idx < nr * w; idx += blockDim.x) {
    const int rl = idx / w, it = idx % w;
    double* o = out + (r0 + rl) * m;
    if (it < ntm) {
      o[it] = tm_inv;
      continue;
    }
    const int k = 2 * (it - ntm);
    double phi[2];
    {
      const double f0 = Ff[k], f1 = Ff[k + 1];
      const double ng = s_ng[0][rl];
      const double p0 = pow(f0, ng);
      const double p1 = (f1 == f0) ? p0 : pow(f1, ng);
      const double a2 = s_a2[0][rl], fy = s_fy[0][rl];
      phi[0] = p0 * a2 * inv12 * invpi2 * fy * dff[k];
      phi[1] = p1 * a2 * inv12 * invpi2 * fy * dff[k + 1];
    }
    if (k < nc) {
      const int k1 = (k + 1 < nc) ? k + 1 : k;
      const double f0 = Ff_c[k], f1 = Ff_c[k1];
      const double ng = s_ng[1][rl];
      const double p0 = pow(f0, ng);
      const double p1 = (f1 == f0) ? p0 : pow(f1, ng);
      const double a2 = s_a2[1][rl], fy = s_fy[1][rl];
      phi[0] = phi[0] + p0 * a2 * inv12 * invpi2 * fy * dff_c[k];
      if (k + 1 < nc)
        phi[1] = phi[1] + p1 * a2 * inv12 * invpi2 * fy * dff_c[k1];
    }
    o[ntm + k] = 1.0 / phi[0];
    o[ntm + k + 1] = 1.0 / phi[1];
  }
}

// ---------------------------------------------------------------------
// host-side launchers (called from bindings.cpp), declared in
// launchers.h.  Each returns the hipError_t of its launch as an int
// (0 = success); a solve dimension with no instantiation is
// hipErrorInvalidValue, never a silent no-op.
// ---------------------------------------------------------------------
extern "C" {

int launch_sigdots(const double* toas, const double* ninv, const double* nr,
                   const double* freqs, int ntoa, int F, double* sNs,
                   double* sNr, hipStream_t stream) {
  hipLaunchKernelGGL(sigdots_kernel, dim3(F), dim3(256), 0, stream, toas,
                     ninv, nr, freqs, ntoa, F, sNs, sNr);
  return (int)hipGetLastError();
}

int launch_sbgemm(const double* T, const double* toas, const double* ninv,
                  const double* freqs, int ntoa, int m, int mp, int F2,
                  double* out, long plane_stride, long ldo, int ksplit,
                  hipStream_t stream) {
  const int ctiles = (F2 + 63) / 64;
  const int mtiles = (mp + FASTFP_MAXMP - 1) / FASTFP_MAXMP;
  hipLaunchKernelGGL(sbgemm_kernel, dim3(ctiles, ksplit, mtiles), dim3(512),
                     0, stream, T, toas, ninv, freqs, ntoa, m, mp, F2, out,
                     plane_stride, ldo);
  return (int)hipGetLastError();
}

// The factor's one dispatch: the diagonal from `phiinv` (P,D,m), or,
// with `phiinv` null, from the strided prior rows (chol_batch_kernel).
static int chol_dispatch(const double* TNT, const double* phiinv, int m,
                         int mp, int D, int P, double* L, double* invd,
                         const double* rows, long rows_ps, long rows_ds,
                         const double* delta0, int lead,
                         hipStream_t stream) {
  // small matrices: 256 threads, so that 5 workgroups per CU (the
  // ~95-VGPR diagonal factor allows 5 waves/SIMD) run their serial
  // chains side by side (128 threads, 7 per CU by LDS: within noise,
  // docs/TUNING_NOTES.md); large: 512 threads for MFMA coverage
  const dim3 grid(D, P), blk(mp <= 64 ? 256 : 512);
  // the identity lead is the stacked compressed system's, mp <= 64;
  // its whole 4-step groups are left out of diagonal block 0
  const int t0 = (rows != nullptr && mp <= 64) ? std::min(lead, 15) / 4 : 0;
  switch ((mp >> 4) | (t0 << 4)) {
#define CHOL_CASE(NBT, T0) \
    case NBT | ((T0 / 4) << 4): \
      hipLaunchKernelGGL((chol_batch_kernel<NBT, T0>), grid, blk, 0, stream, \
                         TNT, phiinv, m, D, L, invd, rows, rows_ps, rows_ds, \
                         delta0, lead); break;
    CHOL_CASE(1, 0) CHOL_CASE(2, 0) CHOL_CASE(3, 0) CHOL_CASE(4, 0)
    CHOL_CASE(5, 0) CHOL_CASE(6, 0) CHOL_CASE(7, 0) CHOL_CASE(8, 0)
    CHOL_CASE(1, 4) CHOL_CASE(2, 4) CHOL_CASE(3, 4) CHOL_CASE(4, 4)
    CHOL_CASE(1, 8) CHOL_CASE(2, 8) CHOL_CASE(3, 8) CHOL_CASE(4, 8)
    CHOL_CASE(1, 12) CHOL_CASE(2, 12) CHOL_CASE(3, 12) CHOL_CASE(4, 12)
#undef CHOL_CASE
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_chol_batch(const double* TNT, const double* phiinv, int m, int mp,
                      int D, int P, double* L, double* invd,
                      hipStream_t stream) {
  return chol_dispatch(TNT, phiinv, m, mp, D, P, L, invd, nullptr, 0, 0,
                       nullptr, 0, stream);
}

int launch_chol_rows(const double* TNT, const double* rows, long rows_ps,
                     long rows_ds, const double* delta0, int lead, int m,
                     int mp, int D, int P, double* L, double* invd,
                     hipStream_t stream) {
  if (rows == nullptr || lead < 0 || lead > m) return (int)hipErrorInvalidValue;
  return chol_dispatch(TNT, nullptr, m, mp, D, P, L, invd, rows, rows_ps,
                       rows_ds, delta0, lead, stream);
}

int launch_phi_inv_batch(const double* gam, const double* lgA,
                         const double* gam_c, const double* lgA_c,
                         int c_dstride, const double* Ff, const double* dff,
                         const double* Ff_c, const double* dff_c, int nf,
                         int nc, int ntm, int P, int D, double fyr,
                         double inv12, double invpi2, double tm_inv,
                         double* out, hipStream_t stream) {
  if (nf < 0 || (nf & 1) || nc < 0 || nc > nf || ntm < 0 || P < 0 || D < 0)
    return (int)hipErrorInvalidValue;
  const long nrows = (long)P * D;
  if (nrows == 0 || ntm + nf == 0) return 0;
  const long nblk = (nrows + PHI_ROWS - 1) / PHI_ROWS;
  if (nblk > 0x7fffffffL) return (int)hipErrorInvalidValue;
  // 10.0 and fyr are run-time values to the kernel, so no part of a
  // pow folds at compile time
  hipLaunchKernelGGL(phi_inv_batch_kernel, dim3((unsigned)nblk), dim3(256), 0,
                     stream, gam, lgA, gam_c, lgA_c, c_dstride, Ff, dff, Ff_c,
                     dff_c, nf, nc, ntm, nrows, D, 10.0, fyr, inv12, invpi2,
                     tm_inv, out);
  return (int)hipGetLastError();
}

// One-draw-per-workgroup solve over (ftiles, D, P): Fp accumulated into
// out (P,D,F), or the five products stored into out (P,D,5,F).
int launch_trsm(int prods, const double* L, const double* invd,
                const double* RHS, const double* sNs, const double* sNr,
                int mp, int F, int D, int P, double gsign, double* out,
                hipStream_t stream) {
  return prods ? launch_one_draw<true>(L, invd, RHS, sNs, sNr, mp, F, D, P,
                                       gsign, out, stream)
               : launch_one_draw<false>(L, invd, RHS, sNs, sNr, mp, F, D, P,
                                        gsign, out, stream);
}

// frequencies per workgroup tile of the draw-looping solve
int trsm_fp_draws_tile_freqs() { return DL_FREQS; }

// Draw-looping solve (mp <= 64), plain stores into out (P,D,F) or, in
// products mode, (P,D,5,F) — the layout and the bits of launch_trsm; the
// planning is launch_draws'.
int launch_trsm_draws(int prods, const double* L, const double* invd,
                      const double* RHS, const double* sNs,
                      const double* sNr, int mp, int F, int D, int P,
                      double gsign, double* out, int draws_per_block,
                      int ncu, int lead, hipStream_t stream) {
  return prods ? launch_draws<true>(L, invd, RHS, sNs, sNr, mp, F, D, P,
                                    gsign, out, draws_per_block, ncu, lead,
                                    stream)
               : launch_draws<false>(L, invd, RHS, sNs, sNr, mp, F, D, P,
                                     gsign, out, draws_per_block, ncu, lead,
                                     stream);
}

int launch_diag_inv(const double* L, int mp, long nblk_total, double* invd,
                    hipStream_t stream) {
  hipLaunchKernelGGL(diag_inv_kernel, dim3((nblk_total + 7) / 8), dim3(512),
                     0, stream, L, mp, nblk_total, invd);
  return (int)hipGetLastError();
}

int launch_sigdots_block(const double* toas, const double* uvec,
                         const double* nr, const double* freqs,
                         const double* beta, const long* offsets,
                         const long* sizes, int nblk, int ntoa, int F,
                         double* sNs, double* sNr, hipStream_t stream) {
  hipLaunchKernelGGL(sigdots_block_kernel, dim3(F), dim3(256), 0, stream,
                     toas, uvec, nr, freqs, beta, offsets, sizes,
                     nblk, ntoa, F, sNs, sNr);
  return (int)hipGetLastError();
}

}  // extern "C"
