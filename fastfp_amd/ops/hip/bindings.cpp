// PyTorch bindings for the fastfp_amd fp64 HIP kernels (MI355X/gfx950).
//
// Thin shape/contiguity-checked wrappers; all launches go onto the
// current torch HIP stream so the ops compose with torch eager code.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <climits>

#include "launchers.h"

namespace {

void check_f64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat64, name, " must be fp64");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

hipStream_t stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// Every launcher returns its hipError_t as an int: an unsupported solve
// dimension or a rejected launch raises instead of leaving the outputs
// unwritten.
void check_launch(int err, const char* what) {
  TORCH_CHECK(err == 0, what, " launch failed: ",
              hipGetErrorString((hipError_t)err));
}

}  // namespace

// sigdots: (toas, ninv, nr (ntoa,), freqs (F,)) -> sNs (3,F), sNr (2,F)
std::vector<torch::Tensor> sigdots(torch::Tensor toas, torch::Tensor ninv,
                                   torch::Tensor nr, torch::Tensor freqs) {
  check_f64(toas, "toas");
  check_f64(ninv, "ninv");
  check_f64(nr, "nr");
  check_f64(freqs, "freqs");
  const int ntoa = toas.size(0);
  const int F = freqs.size(0);
  auto opts = toas.options();
  // no frequencies: empty outputs; no TOAs: every dot is an empty sum
  if (F == 0 || ntoa == 0)
    return {torch::zeros({3, F}, opts), torch::zeros({2, F}, opts)};
  auto sNs = torch::empty({3, F}, opts);
  auto sNr = torch::empty({2, F}, opts);
  check_launch(
      launch_sigdots(toas.data_ptr<double>(), ninv.data_ptr<double>(),
                     nr.data_ptr<double>(), freqs.data_ptr<double>(), ntoa, F,
                     sNs.data_ptr<double>(), sNr.data_ptr<double>(), stream()),
      "sigdots");
  return {sNs, sNr};
}

// sbgemm into `out` (plane-strided), out[j, col0 + c] over F2 columns.
void sbgemm(torch::Tensor T, torch::Tensor toas, torch::Tensor ninv,
            torch::Tensor freqs, torch::Tensor out, int64_t plane_stride,
            int64_t ldo, int64_t mp, int64_t ksplit) {
  check_f64(T, "T");
  check_f64(toas, "toas");
  check_f64(ninv, "ninv");
  check_f64(freqs, "freqs");
  check_f64(out, "out");
  const int ntoa = T.size(0);
  const int m = T.size(1);
  const int F2 = 2 * freqs.size(0);
  TORCH_CHECK(mp % 16 == 0 && mp >= m, "bad mp");  // M-tiled: no upper cap
  TORCH_CHECK(ksplit >= 1, "ksplit must be >= 1");
  if (F2 == 0 || mp == 0) return;  // nothing to write
  if (ntoa == 0) {  // empty K sum: the kernel would store zeros
    out.zero_();
    return;
  }
  check_launch(
      launch_sbgemm(T.data_ptr<double>(), toas.data_ptr<double>(),
                    ninv.data_ptr<double>(), freqs.data_ptr<double>(), ntoa, m,
                    (int)mp, F2, out.data_ptr<double>(), plane_stride, ldo,
                    (int)ksplit, stream()),
      "sbgemm");
}

// chol_batch_into: TNT (m,m) or (P,m,m), phiinv (D,m) or (P,D,m) ->
// caller-owned L (P*D,mp,mp), invd (P*D,mp/16,16,16) (the engine's
// ping-pong pipeline buffers — avoids per-chunk allocator churn across
// streams).
void chol_batch_into(torch::Tensor TNT, torch::Tensor phiinv, int64_t mp,
                     torch::Tensor L, torch::Tensor invd) {
  check_f64(TNT, "TNT");
  check_f64(phiinv, "phiinv");
  check_f64(L, "L");
  check_f64(invd, "invd");
  const bool batched = TNT.dim() == 3;
  const int P = batched ? TNT.size(0) : 1;
  const int m = TNT.size(batched ? 1 : 0);
  const int D = phiinv.size(batched ? 1 : 0);
  TORCH_CHECK(phiinv.dim() == (batched ? 3 : 2), "phiinv rank");
  TORCH_CHECK(phiinv.size(batched ? 2 : 1) == m, "phiinv width != m");
  TORCH_CHECK(mp % 16 == 0 && mp >= 16 && mp <= 128 && mp >= m, "mp");
  TORCH_CHECK(L.size(0) == (long)P * D && L.size(1) == mp && L.size(2) == mp,
              "L shape");
  TORCH_CHECK(invd.size(0) == (long)P * D && invd.size(1) == mp / 16,
              "invd shape");
  if (D == 0 || P == 0) return;  // empty batch: nothing to factor
  check_launch(
      launch_chol_batch(TNT.data_ptr<double>(), phiinv.data_ptr<double>(), m,
                        (int)mp, D, P, L.data_ptr<double>(),
                        invd.data_ptr<double>(), stream()),
      "chol_batch");
}

// chol_rows_into: chol_batch_into with the diagonal read where the phi
// assembly left it.  `row0` is pulsar 0's (D_all, width) view of the prior
// rows (unit column stride); pulsar p's view lies `pstride` elements
// further per pulsar in the same storage.  The factor takes draws
// [d0, d0 + D) and columns [var0, var0 + m - lead) of it: the diagonal is
// 0 on the `lead` leading identity rows of TNT (P,m,m) and behind them
// the row entry, or 1 / (entry - delta0[p]) with delta0 (P, m-lead) given.
// TNT = blockdiag(I_lead, G): the factor relies on that identity block
// (launchers.h).
void chol_rows_into(torch::Tensor TNT, torch::Tensor row0, int64_t pstride,
                    int64_t d0, int64_t D, int64_t var0,
                    c10::optional<torch::Tensor> delta0, int64_t lead,
                    int64_t mp, torch::Tensor L, torch::Tensor invd) {
  check_f64(TNT, "TNT");
  check_f64(L, "L");
  check_f64(invd, "invd");
  TORCH_CHECK(TNT.dim() == 3, "TNT must be (P,m,m)");
  TORCH_CHECK(row0.is_cuda() && row0.scalar_type() == torch::kFloat64 &&
                  row0.dim() == 2 && (row0.size(1) <= 1 || row0.stride(1) == 1),
              "row0 must be a (D,width) fp64 GPU view with unit column stride");
  const int64_t P = TNT.size(0), m = TNT.size(1);
  const int64_t mv = m - lead;
  TORCH_CHECK(TNT.size(2) == m, "TNT must be square");
  TORCH_CHECK(lead >= 0 && mv >= 0, "lead");
  TORCH_CHECK(mp % 16 == 0 && mp >= 16 && mp <= 128 && mp >= m, "mp");
  TORCH_CHECK(D >= 0 && d0 >= 0 && d0 + D <= row0.size(0), "draw range");
  TORCH_CHECK(var0 >= 0 && var0 + mv <= row0.size(1), "column range");
  TORCH_CHECK(pstride >= 0, "pstride");
  TORCH_CHECK(L.size(0) == P * D && L.size(1) == mp && L.size(2) == mp,
              "L shape");
  TORCH_CHECK(invd.size(0) == P * D && invd.size(1) == mp / 16, "invd shape");
  if (D == 0 || P == 0) return;  // empty batch: nothing to factor
  const int64_t dstride = row0.stride(0);
  TORCH_CHECK(dstride >= 0, "row0 draw stride");
  // the last element the kernel reads must lie inside row0's storage
  const int64_t last = row0.storage_offset() + (P - 1) * pstride +
                       (d0 + D - 1) * dstride + var0 + mv - 1;
  TORCH_CHECK(mv == 0 ||
                  (last + 1) * (int64_t)sizeof(double) <=
                      (int64_t)row0.storage().nbytes(),
              "prior rows reach past their storage");
  const double* dl = nullptr;
  if (delta0.has_value()) {
    check_f64(*delta0, "delta0");
    TORCH_CHECK(delta0->dim() == 2 && delta0->size(0) == P &&
                    delta0->size(1) == mv, "delta0 must be (P, m-lead)");
    dl = delta0->data_ptr<double>();
  }
  check_launch(
      launch_chol_rows(TNT.data_ptr<double>(),
                       row0.data_ptr<double>() + d0 * dstride + var0, pstride,
                       dstride, dl, (int)lead, (int)m, (int)mp, (int)D, (int)P,
                       L.data_ptr<double>(), invd.data_ptr<double>(), stream()),
      "chol_rows");
}

// phi_inv_batch: gam, lgA (P,D); the common process gam_c, lgA_c (D,) or
// (1,) on the bins Ff_c, dff_c (nc,) (all four absent: no common
// process); Ff, dff (nf,) -> out (P,D,ntm+nf), every entry written.
void phi_inv_batch(torch::Tensor gam, torch::Tensor lgA,
                   c10::optional<torch::Tensor> gam_c,
                   c10::optional<torch::Tensor> lgA_c, torch::Tensor Ff,
                   torch::Tensor dff, c10::optional<torch::Tensor> Ff_c,
                   c10::optional<torch::Tensor> dff_c, int64_t ntm, double fyr,
                   double inv12, double invpi2, double tm_inv,
                   torch::Tensor out) {
  check_f64(gam, "gam");
  check_f64(lgA, "lgA");
  check_f64(Ff, "Ff");
  check_f64(dff, "dff");
  check_f64(out, "out");
  TORCH_CHECK(gam.dim() == 2 && lgA.sizes() == gam.sizes(),
              "gam, lgA must be (P,D)");
  const int64_t P = gam.size(0), D = gam.size(1), nf = Ff.numel();
  TORCH_CHECK(Ff.dim() == 1 && dff.dim() == 1 && dff.numel() == nf &&
                  nf % 2 == 0, "Ff, dff must be (nf,), nf even");
  TORCH_CHECK(ntm >= 0 && out.dim() == 3 && out.size(0) == P &&
                  out.size(1) == D && out.size(2) == ntm + nf, "out shape");
  TORCH_CHECK(P * D <= INT_MAX && ntm + nf <= INT_MAX / 64, "size");
  int64_t nc = 0, cstride = 0;
  const double *gc = nullptr, *lc = nullptr, *fc = nullptr, *dc = nullptr;
  if (gam_c.has_value()) {
    TORCH_CHECK(lgA_c.has_value() && Ff_c.has_value() && dff_c.has_value(),
                "the common process needs gam_c, lgA_c, Ff_c and dff_c");
    check_f64(*gam_c, "gam_c");
    check_f64(*lgA_c, "lgA_c");
    check_f64(*Ff_c, "Ff_c");
    check_f64(*dff_c, "dff_c");
    nc = Ff_c->numel();
    TORCH_CHECK(Ff_c->dim() == 1 && dff_c->dim() == 1 &&
                    dff_c->numel() == nc && nc <= nf, "Ff_c, dff_c (nc <= nf)");
    const int64_t n = gam_c->numel();
    TORCH_CHECK(gam_c->dim() == 1 && lgA_c->dim() == 1 &&
                    lgA_c->numel() == n && (n == D || n == 1),
                "gam_c, lgA_c must be (D,) or (1,)");
    cstride = (n == 1) ? 0 : 1;
    gc = gam_c->data_ptr<double>();
    lc = lgA_c->data_ptr<double>();
    fc = Ff_c->data_ptr<double>();
    dc = dff_c->data_ptr<double>();
  }
  check_launch(
      launch_phi_inv_batch(gam.data_ptr<double>(), lgA.data_ptr<double>(), gc,
                           lc, (int)cstride, Ff.data_ptr<double>(),
                           dff.data_ptr<double>(), fc, dc, (int)nf, (int)nc,
                           (int)ntm, (int)P, (int)D, fyr, inv12, invpi2, tm_inv,
                           out.data_ptr<double>(), stream()),
      "phi_inv_batch");
}

// chol_batch: allocate L/invd and factor into them.
std::vector<torch::Tensor> chol_batch(torch::Tensor TNT, torch::Tensor phiinv,
                                      int64_t mp) {
  const bool batched = TNT.dim() == 3;
  const int m = TNT.size(batched ? 1 : 0);
  TORCH_CHECK(phiinv.dim() == (batched ? 3 : 2), "phiinv rank");
  TORCH_CHECK(mp % 16 == 0 && mp >= 16 && mp <= 128 && mp >= m,
              "chol_batch requires m <= 128 (solve dimension); got m=", m);
  const long n = (batched ? TNT.size(0) : 1) * phiinv.size(batched ? 1 : 0);
  auto L = torch::empty({n, mp, mp}, TNT.options());
  auto invd = torch::empty({n, mp / 16, 16, 16}, TNT.options());
  chol_batch_into(TNT, phiinv, mp, L, invd);
  return {L, invd};
}

namespace {

struct SolveDims {
  int P, mp, F, D;
};

// Shapes of one solve, shared by the trsm_fp_* and trsm_prods* ops: single
// pulsar (L (D,mp,mp), RHS (mp,2F+1), sNs (3,F), sNr (2,F)) or
// pulsar-batched (L (P*D,mp,mp), RHS (P,mp,2F+1), sNs (P,3,F),
// sNr (P,2,F)).  `out` is (D,[K,]F) / (P,D,[K,]F); K = 0 means no such
// dimension.
SolveDims check_solve(const torch::Tensor& L, const torch::Tensor& invd,
                      const torch::Tensor& RHS, const torch::Tensor& sNs,
                      const torch::Tensor& sNr, const torch::Tensor& out,
                      const char* oname, int K) {
  check_f64(L, "L");
  check_f64(invd, "invd");
  check_f64(RHS, "RHS");
  check_f64(sNs, "sNs");
  check_f64(sNr, "sNr");
  check_f64(out, oname);
  const bool batched = RHS.dim() == 3;
  const int b = batched ? 1 : 0;
  SolveDims d;
  d.P = batched ? RHS.size(0) : 1;
  d.mp = L.size(1);
  d.F = sNs.size(b + 1);
  TORCH_CHECK(out.dim() == b + (K ? 3 : 2), oname, " rank");
  d.D = out.size(b);
  TORCH_CHECK(L.dim() == 3 && L.size(2) == d.mp &&
                  L.size(0) == (long)d.P * d.D,
              "L batch != P*D");
  TORCH_CHECK(invd.numel() == (long)d.P * d.D * d.mp * 16, "invd shape");
  TORCH_CHECK(RHS.size(b) == d.mp && RHS.size(b + 1) == 2 * d.F + 1,
              "RHS shape");
  TORCH_CHECK(sNs.numel() == (long)d.P * 3 * d.F &&
                  sNr.numel() == (long)d.P * 2 * d.F,
              "sNs/sNr shape");
  TORCH_CHECK((!batched || out.size(0) == d.P) &&
                  (!K || out.size(b + 1) == K) &&
                  out.size(out.dim() - 1) == d.F,
              oname, " shape");
  return d;
}

// What tells the four solve ops apart.
struct SolveOp {
  const char* name;     // the Python-visible op
  bool prods;           // five products (out has a K = 5 dimension), not Fp
  bool draws;           // the draw-looping kernel
  int max_mp;           // cap on the padded solve dimension
  const char* instead;  // where the error sends a caller above the cap
};

// The one body of the four solve ops: shapes, the op's mp cap, the
// draw-loop arguments, nothing to do on empty shapes, launch.
void solve(const SolveOp& op, const torch::Tensor& L,
           const torch::Tensor& invd, const torch::Tensor& RHS,
           const torch::Tensor& sNs, const torch::Tensor& sNr,
           const torch::Tensor& out, const char* oname, double gsign,
           int64_t draws_per_block = 0, int64_t lead = 0) {
  const SolveDims d =
      check_solve(L, invd, RHS, sNs, sNr, out, oname, op.prods ? 5 : 0);
  TORCH_CHECK(d.mp % 16 == 0 && d.mp >= 16 && d.mp <= op.max_mp, op.name,
              " supports a padded solve dimension mp <= ", op.max_mp,
              " (multiple of 16); got mp=", d.mp, " — use ", op.instead);
  if (op.draws) {
    TORCH_CHECK(draws_per_block >= 0 && draws_per_block < (1L << 31),
                "draws_per_block must be >= 0");
    TORCH_CHECK(lead >= 0 && lead <= 12 && lead % 4 == 0,
                "lead must be 0, 4, 8 or 12; got ", lead);
  }
  if (d.D == 0 || d.F == 0 || d.P == 0) return;
  if (!op.draws) {
    check_launch(
        launch_trsm(op.prods, L.data_ptr<double>(), invd.data_ptr<double>(),
                    RHS.data_ptr<double>(), sNs.data_ptr<double>(),
                    sNr.data_ptr<double>(), d.mp, d.F, d.D, d.P, gsign,
                    out.data_ptr<double>(), stream()),
        op.name);
    return;
  }
  // the factor is fetched with 16-byte loads
  TORCH_CHECK((reinterpret_cast<uintptr_t>(L.data_ptr<double>()) |
               reinterpret_cast<uintptr_t>(invd.data_ptr<double>())) % 16 == 0,
              "L and invd must be 16-byte aligned");
  const int ncu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  check_launch(
      launch_trsm_draws(op.prods, L.data_ptr<double>(),
                        invd.data_ptr<double>(), RHS.data_ptr<double>(),
                        sNs.data_ptr<double>(), sNr.data_ptr<double>(), d.mp,
                        d.F, d.D, d.P, gsign, out.data_ptr<double>(),
                        (int)draws_per_block, ncu, (int)lead, stream()),
      op.name);
}

}  // namespace

// trsm_fp_accum: solve + fused 2x2 reduction, accumulating in place
// into fp (D,F) / (P,D,F).
void trsm_fp_accum(torch::Tensor L, torch::Tensor invd, torch::Tensor RHS,
                   torch::Tensor sNs, torch::Tensor sNr, torch::Tensor fp,
                   double gsign) {
  solve({"trsm_fp_accum", false, false, 256,
         "the Schur-compressed system or the CPU engine"},
        L, invd, RHS, sNs, sNr, fp, "fp", gsign);
}

// trsm_fp_store: the same solve and reduction as trsm_fp_accum for
// mp <= 64, by the draw-looping kernel: a workgroup keeps its RHS tile
// in registers over `draws_per_block` consecutive draws (0: sized from
// the device's resident workgroup slots).  Plain stores: every entry of
// `out` (D,F) / (P,D,F) is written and none is read, so `out` need not
// be initialised; the values equal trsm_fp_accum into zeros bit for bit.
// `lead` (0, 4, 8 or 12) promises that the first `lead` rows of RHS are
// zero and that the system starts with a `lead` x `lead` identity block
// (L[lead:, :lead] = 0): the kernel then leaves out the MFMAs that would
// multiply those zeros, and the result keeps every bit of lead = 0.
void trsm_fp_store(torch::Tensor L, torch::Tensor invd, torch::Tensor RHS,
                   torch::Tensor sNs, torch::Tensor sNr, torch::Tensor out,
                   double gsign, int64_t draws_per_block, int64_t lead) {
  solve({"trsm_fp_store", false, true, 64, "trsm_fp_accum"}, L, invd, RHS,
        sNs, sNr, out, "out", gsign, draws_per_block, lead);
}

// trsm_prods: the same solve as trsm_fp_accum, but the five corrected
// products [ss, cc, sc, sr, cr] are stored un-collapsed: out (D,5,F)
// for a single pulsar, (P,D,5,F) pulsar-batched.  Plain stores — `out`
// need not be zeroed.
void trsm_prods(torch::Tensor L, torch::Tensor invd, torch::Tensor RHS,
                torch::Tensor sNs, torch::Tensor sNr, torch::Tensor out,
                double gsign) {
  solve({"trsm_prods", true, false, 128,
         "FpEngine.sweep_products for larger bases"},
        L, invd, RHS, sNs, sNr, out, "out", gsign);
}

// trsm_prods_store: the five products of trsm_prods for mp <= 64, by the
// products mode of the draw-looping kernel (see trsm_fp_store for
// `draws_per_block` and `lead`).  Plain stores: every entry of `out`
// (D,5,F) / (P,D,5,F) is written and none is read; the values equal
// trsm_prods on the same L/invd/RHS bit for bit.
void trsm_prods_store(torch::Tensor L, torch::Tensor invd, torch::Tensor RHS,
                      torch::Tensor sNs, torch::Tensor sNr, torch::Tensor out,
                      double gsign, int64_t draws_per_block, int64_t lead) {
  solve({"trsm_prods_store", true, true, 64, "trsm_prods"}, L, invd, RHS, sNs,
        sNr, out, "out", gsign, draws_per_block, lead);
}

namespace {

// dtype, shape and device checks common to every Fe kernel
void check_fe_shapes(const torch::Tensor& prods, const torch::Tensor& ant) {
  check_f64(prods, "prods");
  check_f64(ant, "ant");
  TORCH_CHECK(prods.dim() == 4 && prods.size(2) == 5,
              "prods must be (P, D, 5, F)");
  TORCH_CHECK(ant.dim() == 3 && ant.size(2) == 2 &&
                  ant.size(1) == prods.size(0),
              "ant must be (nsky, P, 2) with P matching prods");
  TORCH_CHECK(ant.device() == prods.device(), "prods/ant device mismatch");
}

void check_fe_dims(const torch::Tensor& prods, const torch::Tensor& ant) {
  TORCH_CHECK(prods.size(3) < (1L << 31) && ant.size(0) < (1L << 31) &&
                  prods.size(1) < (1L << 31),
              "dimension overflow");
}

void check_fe_inputs(const torch::Tensor& prods, const torch::Tensor& ant) {
  check_fe_shapes(prods, ant);
  TORCH_CHECK(prods.size(0) >= 1 && prods.size(0) <= fe_max_pulsars(),
              "the Fe sky kernels keep a (5, P, 16) product tile in LDS and "
              "support 1 <= P <= ", fe_max_pulsars(), " pulsars; got P=",
              prods.size(0));
  check_fe_dims(prods, ant);
}

}  // namespace

// fe_amplitudes: the 4x4 solve at ONE sky row idx (D,F) i32 per column ->
// amps (D,F,4) = M^-1 N, fe (D,F), status (D,F) i32: 0 solved, 1
// degenerate pivot, 2 idx outside [0, nsky); NaN where status != 0.  No
// pulsar cap: the kernel keeps no product tile.
std::vector<torch::Tensor> fe_amplitudes(torch::Tensor prods,
                                         torch::Tensor ant,
                                         torch::Tensor idx) {
  check_fe_shapes(prods, ant);
  TORCH_CHECK(prods.size(0) >= 1 && prods.size(0) < (1L << 31),
              "fe_amplitudes needs P >= 1 pulsars; got P=", prods.size(0));
  check_fe_dims(prods, ant);
  TORCH_CHECK(idx.is_cuda() && idx.device() == prods.device(),
              "idx must be on the device of prods");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32, "idx must be int32");
  TORCH_CHECK(idx.is_contiguous(), "idx must be contiguous");
  TORCH_CHECK(idx.dim() == 2 && idx.size(0) == prods.size(1) &&
                  idx.size(1) == prods.size(3),
              "idx must be (D, F) matching prods");
  const int P = prods.size(0), D = prods.size(1), F = prods.size(3);
  const int nsky = ant.size(0);
  auto iopts = prods.options().dtype(torch::kInt32);
  auto amps = torch::empty({D, F, 4}, prods.options());
  auto fe = torch::empty({D, F}, prods.options());
  auto status = torch::empty({D, F}, iopts);
  check_launch(
      launch_fe_amplitudes(prods.data_ptr<double>(), ant.data_ptr<double>(),
                           idx.data_ptr<int>(), P, D, F, nsky,
                           amps.data_ptr<double>(), fe.data_ptr<double>(),
                           status.data_ptr<int>(), stream()),
      "fe_amplitudes");
  return {amps, fe, status};
}

// fe_assemble: prods (P,D,5,F), ant (nsky,P,2) -> fe (D,nsky,F); NaN at
// points whose 4x4 M has a degenerate Cholesky pivot.
torch::Tensor fe_assemble(torch::Tensor prods, torch::Tensor ant) {
  check_fe_inputs(prods, ant);
  const int P = prods.size(0), D = prods.size(1), F = prods.size(3);
  const int nsky = ant.size(0);
  auto fe = torch::empty({D, nsky, F}, prods.options());
  check_launch(
      launch_fe_assemble(prods.data_ptr<double>(), ant.data_ptr<double>(), P,
                         D, F, nsky, fe.data_ptr<double>(), stream()),
      "fe_assemble");
  return fe;
}

// fe_skymax: running maximum over the sky inside the kernel ->
// femax (D,F) f64, argmax (D,F) i32 (lowest index on ties, -1 if every
// point was skipped), nskip (D,F) i32 = degenerate points left out.
std::vector<torch::Tensor> fe_skymax(torch::Tensor prods, torch::Tensor ant) {
  check_fe_inputs(prods, ant);
  const int P = prods.size(0), D = prods.size(1), F = prods.size(3);
  const int nsky = ant.size(0);
  auto iopts = prods.options().dtype(torch::kInt32);
  auto femax = torch::full({D, F}, -INFINITY, prods.options());
  auto argmax = torch::full({D, F}, -1, iopts);
  auto nskip = torch::zeros({D, F}, iopts);
  check_launch(
      launch_fe_skymax(prods.data_ptr<double>(), ant.data_ptr<double>(), P, D,
                       F, nsky, femax.data_ptr<double>(),
                       argmax.data_ptr<int>(), nskip.data_ptr<int>(),
                       stream()),
      "fe_skymax");
  return {femax, argmax, nskip};
}

// fe_mfactor: the LDL^T of every (column, sky) 4x4 M as the sky kernels
// factor it -> fac (D, F, nsky, 10) = [l10, l20, l30, l21, l31, l32, 1/d0,
// 1/d1, 1/d2, 1/d3]; ten NaNs at the points they skip.  Reads only the
// planes ss, cc, sc of prods.
torch::Tensor fe_mfactor(torch::Tensor prods, torch::Tensor ant) {
  check_fe_inputs(prods, ant);
  const int P = prods.size(0), D = prods.size(1), F = prods.size(3);
  const int nsky = ant.size(0);
  auto fac = torch::empty({D, F, nsky, fe_null_fac_numbers()},
                          prods.options());
  check_launch(
      launch_fe_mfactor(prods.data_ptr<double>(), ant.data_ptr<double>(), P,
                        D, F, nsky, fac.data_ptr<double>(), stream()),
      "fe_mfactor");
  return fac;
}

// fe_null_skymax: the sky maximum of R noise-only realisations per
// column.  lfac (D,F,P,3) = Cholesky factors [l00, l10, l11] of the
// per-pulsar blocks [[ss, sc], [sc, cc]], z (D,F,P,2,R) standard normals
// -> femax (D,F,R) f64, argmax (D,F,R) i32 (lowest index on ties, -1 and
// -inf if every point was skipped), nskip (D,F) i32.
std::vector<torch::Tensor> fe_null_skymax(torch::Tensor prods,
                                          torch::Tensor ant,
                                          torch::Tensor lfac, torch::Tensor z,
                                          int64_t rtiles) {
  check_fe_shapes(prods, ant);
  TORCH_CHECK(prods.size(0) >= 1 && prods.size(0) <= fe_max_pulsars(),
              "the Fe null kernel keeps a (2, P, 16) realisation tile in LDS "
              "next to the sky kernels' factor pass and supports 1 <= P <= ",
              fe_max_pulsars(), " pulsars; got P=", prods.size(0));
  check_fe_dims(prods, ant);
  check_f64(lfac, "lfac");
  check_f64(z, "z");
  const int P = prods.size(0), D = prods.size(1), F = prods.size(3);
  const int nsky = ant.size(0);
  TORCH_CHECK(lfac.device() == prods.device() && z.device() == prods.device(),
              "prods/lfac/z device mismatch");
  TORCH_CHECK(lfac.dim() == 4 && lfac.size(0) == D && lfac.size(1) == F &&
                  lfac.size(2) == P && lfac.size(3) == 3,
              "lfac must be (D, F, P, 3) matching prods");
  TORCH_CHECK(z.dim() == 5 && z.size(0) == D && z.size(1) == F &&
                  z.size(2) == P && z.size(3) == 2,
              "z must be (D, F, P, 2, R) matching prods");
  TORCH_CHECK(z.size(4) < (1L << 31), "dimension overflow");
  TORCH_CHECK(rtiles == 0 || rtiles == 1 || rtiles == 2 || rtiles == 4,
              "rtiles must be 0 (default), 1, 2 or 4");
  const int R = z.size(4);
  auto iopts = prods.options().dtype(torch::kInt32);
  auto femax = torch::full({D, F, R}, -INFINITY, prods.options());
  auto argmax = torch::full({D, F, R}, -1, iopts);
  auto nskip = torch::zeros({D, F}, iopts);
  auto fac = torch::empty({D, F, nsky, fe_null_fac_numbers()},
                          prods.options());
  check_launch(
      launch_fe_null_skymax(prods.data_ptr<double>(), ant.data_ptr<double>(),
                            lfac.data_ptr<double>(), z.data_ptr<double>(), P,
                            D, F, nsky, R, (int)rtiles,
                            fac.data_ptr<double>(), femax.data_ptr<double>(),
                            argmax.data_ptr<int>(), nskip.data_ptr<int>(),
                            stream()),
      "fe_null_skymax");
  return {femax, argmax, nskip};
}

// fe_null_data: joint null data n = white^T - rhs^T X per (pulsar, draw),
// written into `out` (D, F, P, 2, R), the z layout of fe_null_skymax.
// white (P, Rp, ldw) is taken AS sbgemm WRITES IT, white[p][r][2f+c] with
// Rp >= R rows and ldw >= 2F columns: the kernel transposes it while it
// loads the accumulators.  rhs (P, mp, 2F+1) is the engine's stacked RHS
// (last column not read); X (P, D, mp, R) must hold zeros in the padding
// rows.  `out` may be a larger buffer's leading part: exactly its
// D*F*P*2*R entries are written.
void fe_null_data(torch::Tensor white, torch::Tensor rhs, torch::Tensor X,
                  torch::Tensor out) {
  check_f64(white, "white");
  check_f64(rhs, "rhs");
  check_f64(X, "X");
  check_f64(out, "out");
  TORCH_CHECK(white.device() == rhs.device() && X.device() == rhs.device() &&
                  out.device() == rhs.device(),
              "white/rhs/X/out device mismatch");
  TORCH_CHECK(rhs.dim() == 3 && rhs.size(2) >= 1 && rhs.size(2) % 2 == 1,
              "rhs must be (P, mp, 2F+1)");
  const int64_t P = rhs.size(0), mp = rhs.size(1), F = (rhs.size(2) - 1) / 2;
  TORCH_CHECK(mp % 16 == 0 && mp >= 16 && mp <= 256,
              "fe_null_data supports mp = a multiple of 16 up to 256; got ",
              mp);
  TORCH_CHECK(X.dim() == 4 && X.size(0) == P && X.size(2) == mp,
              "X must be (P, D, mp, R) matching rhs");
  const int64_t D = X.size(1), R = X.size(3);
  TORCH_CHECK(white.dim() == 3 && white.size(0) == P && white.size(1) >= R &&
                  white.size(2) >= 2 * F,
              "white must be (P, Rp >= R, ldw >= 2F) matching rhs and X");
  TORCH_CHECK(out.dim() == 5 && out.size(0) == D && out.size(1) == F &&
                  out.size(2) == P && out.size(3) == 2 && out.size(4) == R,
              "out must be (D, F, P, 2, R)");
  TORCH_CHECK(P < (1L << 31) && D < (1L << 31) && F < (1L << 30) &&
                  R < (1L << 31) && white.size(1) < (1L << 31) &&
                  white.size(2) < (1L << 31),
              "dimension overflow");
  check_launch(
      launch_fe_null_data(white.data_ptr<double>(), rhs.data_ptr<double>(),
                          X.data_ptr<double>(), (int)P, (int)D, (int)F, (int)R,
                          (int)white.size(1), (int)white.size(2), (int)mp,
                          out.data_ptr<double>(), stream()),
      "fe_null_data");
}

// diag_inv: invert the 16x16 diagonal blocks of batched lower-tri L
// (B, mp, mp) -> invd (B, mp/16, 16, 16); the m > 128 direct path.
torch::Tensor diag_inv(torch::Tensor L) {
  check_f64(L, "L");
  TORCH_CHECK(L.dim() == 3 && L.size(1) == L.size(2), "L must be (B,mp,mp)");
  const long B = L.size(0);
  const int mp = L.size(1);
  TORCH_CHECK(mp % 16 == 0, "mp multiple of 16");
  auto invd = torch::empty({B, mp / 16, 16, 16}, L.options());
  if (B == 0 || mp == 0) return invd;  // no blocks
  check_launch(launch_diag_inv(L.data_ptr<double>(), mp, B * (mp / 16),
                               invd.data_ptr<double>(), stream()),
               "diag_inv");
  return invd;
}

// sigdots_block: Sherman-Morrison block-diagonal-N dots.
// toas/uvec/nr (ntoa, permuted), beta (nblk), offsets/sizes (int64).
std::vector<torch::Tensor> sigdots_block(torch::Tensor toas, torch::Tensor uvec,
                                         torch::Tensor nr, torch::Tensor freqs,
                                         torch::Tensor beta,
                                         torch::Tensor offsets,
                                         torch::Tensor sizes) {
  check_f64(toas, "toas");
  check_f64(uvec, "uvec");
  check_f64(nr, "nr");
  check_f64(freqs, "freqs");
  check_f64(beta, "beta");
  const int ntoa = toas.size(0);
  const int F = freqs.size(0);
  const int nblk = sizes.size(0);
  auto opts = toas.options();
  if (F == 0 || ntoa == 0)
    return {torch::zeros({3, F}, opts), torch::zeros({2, F}, opts)};
  auto sNs = torch::empty({3, F}, opts);
  auto sNr = torch::empty({2, F}, opts);
  check_launch(
      launch_sigdots_block(toas.data_ptr<double>(), uvec.data_ptr<double>(),
                           nr.data_ptr<double>(), freqs.data_ptr<double>(),
                           beta.data_ptr<double>(), offsets.data_ptr<long>(),
                           sizes.data_ptr<long>(), nblk, ntoa, F,
                           sNs.data_ptr<double>(), sNr.data_ptr<double>(),
                           stream()),
      "sigdots_block");
  return {sNs, sNr};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sigdots_block", &sigdots_block,
        "fused sincos dots with block-diagonal N (Sherman-Morrison)");
  m.def("diag_inv", &diag_inv,
        "invert 16x16 diagonal blocks of batched lower-triangular L");
  m.def("sigdots", &sigdots, "fused sincos signal-basis dots");
  m.def("sbgemm", &sbgemm, "fused signal-basis MFMA fp64 DGEMM");
  m.def("chol_batch", &chol_batch, "batched LDS-resident fp64 Cholesky");
  m.def("chol_batch_into", &chol_batch_into,
        "chol_batch into caller-owned L/invd (pipeline buffers)");
  m.def("chol_rows_into", &chol_rows_into,
        "chol_batch_into with the diagonal read from strided prior rows",
        py::arg("TNT"), py::arg("row0"), py::arg("pstride"), py::arg("d0"),
        py::arg("D"), py::arg("var0"), py::arg("delta0"), py::arg("lead"),
        py::arg("mp"), py::arg("L"), py::arg("invd"));
  m.def("phi_inv_batch", &phi_inv_batch,
        "homogeneous prior phi^-1 (P,D,ntm+nf) in one kernel");
  m.def("trsm_fp_accum", &trsm_fp_accum,
        "batched TRSM + fused 2x2 Fp reduction");
  m.def("trsm_fp_store", &trsm_fp_store,
        "draw-looping TRSM + fused 2x2 Fp reduction, plain stores (mp <= 64)",
        py::arg("L"), py::arg("invd"), py::arg("RHS"), py::arg("sNs"),
        py::arg("sNr"), py::arg("out"), py::arg("gsign"),
        py::arg("draws_per_block") = 0, py::arg("lead") = 0);
  m.def("trsm_fp_store_tile_freqs", &trsm_fp_draws_tile_freqs,
        "frequencies per workgroup tile of trsm_fp_store");
  m.def("trsm_prods", &trsm_prods,
        "batched TRSM storing the five corrected products (Fe input)");
  m.def("trsm_prods_store", &trsm_prods_store,
        "draw-looping TRSM storing the five corrected products (mp <= 64)",
        py::arg("L"), py::arg("invd"), py::arg("RHS"), py::arg("sNs"),
        py::arg("sNr"), py::arg("out"), py::arg("gsign"),
        py::arg("draws_per_block") = 0, py::arg("lead") = 0);
  m.def("fe_assemble", &fe_assemble,
        "Fe sky assembly: MFMA pulsar sums + in-register 4x4 solve");
  m.def("fe_skymax", &fe_skymax,
        "Fe sky assembly fused with the maximum over sky points");
  m.def("fe_amplitudes", &fe_amplitudes,
        "Fe maximum-likelihood amplitudes at one sky index per column");
  m.def("fe_mfactor", &fe_mfactor,
        "LDL^T factors of the Fe 4x4 M per (column, sky) point");
  m.def("fe_null_skymax", &fe_null_skymax,
        "sky maximum of Fe over noise-only realisations n = L z",
        py::arg("prods"), py::arg("ant"), py::arg("lfac"), py::arg("z"),
        py::arg("rtiles") = 0);
  m.def("fe_null_data", &fe_null_data,
        "joint null data n = white^T - rhs^T X into (D, F, P, 2, R)",
        py::arg("white"), py::arg("rhs"), py::arg("X"), py::arg("out"));
  m.def("fe_max_pulsars", &fe_max_pulsars,
        "largest pulsar count of the Fe sky kernels");
}
