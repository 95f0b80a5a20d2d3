// Operand views of the BatchNorm launchers and the plan walk (net.hip): each names ONE layout or tensor convention once, so a launch site says
// WHICH BatchNorm / statistics record it means and not where its four arrays start.  Host-side only; the launchers unpack them into kernel arguments.
#pragma once
namespace rdm {

// indices of one BatchNorm's tensors in the tensor list of a plan (net.hip Registry)
struct BnIdx { int w, b, rm, rv, nbt; };

// what a finalisation writes and backward reads.  As a workspace record: [scale | shift | mean | rstd] x C floats
struct BnAffine {
  float *scale, *shift, *mean, *rstd;
  BnAffine(float* base, int C) : scale(base), shift(base + C), mean(base + 2 * C), rstd(base + 3 * C) {}
  BnAffine(float* scale_, float* shift_, float* mean_, float* rstd_) : scale(scale_), shift(shift_), mean(mean_), rstd(rstd_) {}      // four loose arrays (C ABI)
  BnAffine at(int c_lo) const { return BnAffine(scale + c_lo, shift + c_lo, mean + c_lo, rstd + c_lo); }                               // channels [c_lo, ...)
};

// a pair of per-channel float64 sums.  As a workspace record: [sum | sumsq] (forward) or [sum dz | sum dz*x] (backward), the second `ld` doubles behind the first
struct StatPair {
  double *sum, *sq;
  StatPair() : sum(nullptr), sq(nullptr) {}                    // eval-mode finalisation reads none
  StatPair(double* base, int ld) : sum(base), sq(base + ld) {}
  StatPair(double* sum_, double* sq_) : sum(sum_), sq(sq_) {}
  StatPair at(int c_lo) const { return StatPair(sum + c_lo, sq + c_lo); }
};

// the tensors of a BatchNorm module.  nbt (num_batches_tracked) is null where the launch must not count a batch: a finalisation of a channel RANGE
// that another launch of the same forward completes, and eval mode
struct BnParams {
  const float *gamma, *beta;
  float *rm, *rv;
  long long* nbt;
  BnParams() : gamma(nullptr), beta(nullptr), rm(nullptr), rv(nullptr), nbt(nullptr) {}
  BnParams(const float* gamma_, const float* beta_, float* rm_, float* rv_, long long* nbt_) : gamma(gamma_), beta(beta_), rm(rm_), rv(rv_), nbt(nbt_) {}
  BnParams(void* const* T, const BnIdx& i, bool count_batch = true)
      : gamma(static_cast<float*>(T[i.w])), beta(static_cast<float*>(T[i.b])), rm(static_cast<float*>(T[i.rm])), rv(static_cast<float*>(T[i.rv])),
        nbt(count_batch ? static_cast<long long*>(T[i.nbt]) : nullptr) {}
  BnParams at(int c_lo, bool count_batch = true) const { return BnParams(gamma + c_lo, beta + c_lo, rm + c_lo, rv + c_lo, count_batch ? nbt : nullptr); }
};

// the gradient slots of a BatchNorm's weight and bias: null where the caller gave none (Gr itself may be null: forward)
struct BnGrads {
  float *dgamma, *dbeta;
  BnGrads(float* dgamma_, float* dbeta_) : dgamma(dgamma_), dbeta(dbeta_) {}
  BnGrads(void* const* Gr, const BnIdx& i) : dgamma(Gr ? static_cast<float*>(Gr[i.w]) : nullptr), dbeta(Gr ? static_cast<float*>(Gr[i.b]) : nullptr) {}
};

}  // namespace rdm
