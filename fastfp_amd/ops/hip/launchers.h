// Host-side launchers of the fastfp_amd HIP kernels: the one declaration
// that the definitions (fastfp_kernels.hip, fe_kernels.hip) and the
// caller (bindings.cpp) all include.  extern "C" names are not mangled,
// so without it a drifted signature would still link; with it a
// definition that disagrees with its declaration does not compile.
//
// Every launcher enqueues on `stream` and returns the hipError_t of its
// launch as an int (0 = success); a solve dimension with no
// instantiation is hipErrorInvalidValue, never a silent no-op.  All
// pointers are device pointers to contiguous fp64 unless typed otherwise.
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

// toas/ninv/nr (ntoa,), freqs (F,) -> sNs (3,F), sNr (2,F)
int launch_sigdots(const double* toas, const double* ninv, const double* nr,
                   const double* freqs, int ntoa, int F, double* sNs,
                   double* sNr, hipStream_t stream);

// sigdots for block-diagonal N: toas/uvec/nr (ntoa,) in block order,
// beta/offsets/sizes (nblk,) -> sNs (3,F), sNr (2,F)
int launch_sigdots_block(const double* toas, const double* uvec,
                         const double* nr, const double* freqs,
                         const double* beta, const long* offsets,
                         const long* sizes, int nblk, int ntoa, int F,
                         double* sNs, double* sNr, hipStream_t stream);

// T (ntoa,m), toas/ninv (ntoa,), freqs (F2/2,) -> out[plane][j][c] for
// j < mp, c < F2, with row stride ldo and one plane (plane_stride apart)
// per K split
int launch_sbgemm(const double* T, const double* toas, const double* ninv,
                  const double* freqs, int ntoa, int m, int mp, int F2,
                  double* out, long plane_stride, long ldo, int ksplit,
                  hipStream_t stream);

// TNT (P,m,m), phiinv (P,D,m) -> L (P*D,mp,mp), invd (P*D,mp/16,16,16);
// mp = 16..128
int launch_chol_batch(const double* TNT, const double* phiinv, int m, int mp,
                      int D, int P, double* L, double* invd,
                      hipStream_t stream);

// The same factor with the diagonal read from strided prior rows: entry
// (p, d, i) at rows[p * rows_ps + d * rows_ds + i], i < m - lead.  The
// diagonal added to TNT (P,m,m) is 0 on its `lead` leading identity rows
// and behind them rows[i], or 1 / (rows[i] - delta0[p][i]) with delta0
// (P, m-lead) not null.  TNT must carry the identity on those `lead` rows
// and columns: for mp <= 64 the factor leaves their whole 4-step groups
// out of diagonal block 0 instead of computing sqrt(1) and x * 0.
int launch_chol_rows(const double* TNT, const double* rows, long rows_ps,
                     long rows_ds, const double* delta0, int lead, int m,
                     int mp, int D, int P, double* L, double* invd,
                     hipStream_t stream);

// Homogeneous prior phi^-1: gam, lgA (P,D); the common process gam_c,
// lgA_c (one entry per draw, c_dstride apart; read only when nc > 0) on
// its own bins Ff_c, dff_c (nc,), nc <= nf; Ff, dff (nf,), nf even ->
// out (P,D,ntm+nf), the first ntm columns tm_inv.  inv12, invpi2: the
// rounded reciprocals of 12 and pi^2 that the power law multiplies by.
int launch_phi_inv_batch(const double* gam, const double* lgA,
                         const double* gam_c, const double* lgA_c,
                         int c_dstride, const double* Ff, const double* dff,
                         const double* Ff_c, const double* dff_c, int nf,
                         int nc, int ntm, int P, int D, double fyr,
                         double inv12, double invpi2, double tm_inv,
                         double* out, hipStream_t stream);

// L (B,mp,mp) -> invd, nblk_total = B * mp/16 inverted diagonal blocks
int launch_diag_inv(const double* L, int mp, long nblk_total, double* invd,
                    hipStream_t stream);

// The solve, one draw per workgroup: L (P*D,mp,mp), invd
// (P*D,mp/16,16,16), RHS (P,mp,2F+1), sNs (P,3,F), sNr (P,2,F).
// prods = 0: Fp ACCUMULATED into out (P,D,F), mp = 16..256;
// prods = 1: the five products stored into out (P,D,5,F), mp = 16..128.
int launch_trsm(int prods, const double* L, const double* invd,
                const double* RHS, const double* sNs, const double* sNr,
                int mp, int F, int D, int P, double gsign, double* out,
                hipStream_t stream);

// The same solve with the loop over draws inside the workgroup, mp =
// 16..64, plain stores in both modes (out as above).  draws_per_block
// = 0 sizes the slice of draws from the resident workgroup slots of
// `ncu` compute units; lead (0, 4, 8 or 12) = leading identity rows of
// the system whose k-steps are left out.
int launch_trsm_draws(int prods, const double* L, const double* invd,
                      const double* RHS, const double* sNs,
                      const double* sNr, int mp, int F, int D, int P,
                      double gsign, double* out, int draws_per_block,
                      int ncu, int lead, hipStream_t stream);

// frequencies per workgroup tile of launch_trsm_draws
int trsm_fp_draws_tile_freqs();

// largest P of the Fe sky kernels
int fe_max_pulsars();

// prods (P,D,5,F), ant (nsky,P,2) -> fe (D,nsky,F)
int launch_fe_assemble(const double* prods, const double* ant, int P, int D,
                       int F, int nsky, double* fe, hipStream_t stream);

// prods (P,D,5,F), ant (nsky,P,2) -> femax, argmax, nskip (D,F); the
// caller initialises the three outputs
int launch_fe_skymax(const double* prods, const double* ant, int P, int D,
                     int F, int nsky, double* femax, int* argmax, int* nskip,
                     hipStream_t stream);

// prods (P,D,5,F), ant (nsky,P,2), idx (D,F) sky row per column -> amps
// (D,F,4) = M^-1 N, fe (D,F), status (D,F): 0 solved, 1 degenerate pivot,
// 2 idx outside [0, nsky); NaN where status != 0.  Any P >= 1.
int launch_fe_amplitudes(const double* prods, const double* ant,
                         const int* idx, int P, int D, int F, int nsky,
                         double* amps, double* fe, int* status,
                         hipStream_t stream);

// numbers per (column, sky) point of the stored M factor
int fe_null_fac_numbers();

// prods (P,D,5,F) planes ss, cc, sc and ant (nsky,P,2) -> fac
// (D*F, nsky, fe_null_fac_numbers()): the LDL^T of every 4x4 M as the
// sky kernels factor it, NaN where they skip the point
int launch_fe_mfactor(const double* prods, const double* ant, int P, int D,
                      int F, int nsky, double* fac, hipStream_t stream);

// Null sky maximum: launch_fe_mfactor into the caller's scratch `fac`,
// then per realisation r the maximum over sky of Fe with N built from
// n = lfac z.  lfac (D,F,P,3) = [l00, l10, l11], z (D,F,P,2,R) -> femax,
// argmax (D,F,R), nskip (D,F); the caller initialises the three outputs.
// rtiles = realisation tiles per workgroup (1, 2 or 4; 0 = the default);
// the launcher lowers it to what R fills and the LDS holds, and no
// result depends on it.
int launch_fe_null_skymax(const double* prods, const double* ant,
                          const double* lfac, const double* z, int P, int D,
                          int F, int nsky, int R, int rtiles, double* fac,
                          double* femax, int* argmax, int* nskip,
                          hipStream_t stream);

// Joint null data: white (P,Rp,ldw) with white[p][r][2f+c] (the kernel
// transposes it), rhs (P,mp,2F+1) whose last column is not read, X
// (P,D,mp,R) with zero padding rows -> out (D,F,P,2,R) =
// white[p][r][2f+c] - sum_k rhs[p][k][2f+c] X[p][d][k][r].  mp = any
// multiple of 16 up to 256; Rp >= R, ldw >= 2F.  Every entry of out is
// written, nothing else.
int launch_fe_null_data(const double* white, const double* rhs,
                        const double* X, int P, int D, int F, int R, int Rp,
                        int ldw, int mp, double* out, hipStream_t stream);

}  // extern "C"
