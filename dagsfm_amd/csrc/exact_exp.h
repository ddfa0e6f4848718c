// exact_exp.h -- exp(x) restated so that the device, the host and tests/patch_match_ref.py compute THE SAME float.
//
// PatchMatch (patch_match.hip) calls exp in ComputeNCCProb and ComputeIncProb
// (the reference's src/mvs/patch_match_cuda.cu:631-653).  The reference evaluates them with CUDA's fast-math __expf, which no
// other machine reproduces; the contract is the mathematically defined value, as for exact_trig.h: the float nearest to
// exp(x).  dsm_exp returns exp(x) in double with an error below one double ulp (Cody-Waite reduction by ln 2 in two parts, the
// Taylor polynomial of degree 13 on |r| <= ln 2 / 2, whose truncation is below 2^-57, scaling by an exact power of two), so its
// rounding to float is the correctly rounded float except where exp(x) lies within 2^-29 float ulps of a rounding boundary.
// tests/test_patch_match_cpu.py holds the host build of this header to glibc's exp rounded to float on 10^6 arguments of
// [-60, 0], with equality.
//
// Plain IEEE double operations in a fixed order, no FMA (both builds use -ffp-contract=off): g++ and hipcc return identical
// bits.  The includer defines DSM_XE, the function qualifier (host: `static inline`; device: `static __host__ __device__ inline`).
#ifndef DAGSFM_AMD_CSRC_EXACT_EXP_H_
#define DAGSFM_AMD_CSRC_EXACT_EXP_H_

DSM_XE double dsm_exp(double x) {
  if (!(x == x)) return x;                      // NaN
  if (x > 709.0) return __builtin_inf();        // exp overflows at 709.78; the callers' arguments are <= 0
  if (x < -708.0) return 0.0;                   // below the normal doubles; every float rounding of it is 0 from -104 on
  const double kInvLn2 = 0x1.71547652b82fep+0;
  const double kLn2Hi = 0x1.62e42fee00000p-1;   // 32 significant bits: k * kLn2Hi is exact for |k| < 2^20
  const double kLn2Lo = 0x1.a39ef35793c76p-33;
  const double t = x * kInvLn2;
  const double k = (t >= 0.0) ? (double)(long long)(t + 0.5) : -(double)(long long)(0.5 - t);
  const double r = (x - k * kLn2Hi) - k * kLn2Lo;
  double p = 1.0 / 6227020800.0;                // 1 / 13!; every 1 / n! below is the correctly rounded quotient of two exact doubles
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const unsigned long long bits = (unsigned long long)((long long)k + 1023) << 52;  // 2^k, -1022 <= k <= 1023
  double scale;
  __builtin_memcpy(&scale, &bits, sizeof(scale));
  return p * scale;
}

#endif  // DAGSFM_AMD_CSRC_EXACT_EXP_H_
