// EC-NTT: the inverse DFT of n = 2^log_n G1 points,
//   out[i] = (1/n) sum_j omega^(-ij) in[j],
// which turns the canonical KZG SRS [tau^j]G into the Lagrange one [L_i(tau)]G
// (kzg.ToLagrangeG1, backend/plonk/bls12-381/setup.go:134).  Both PlonK curves.
//
//   load       affine -> an XYZZ working buffer (so `in` and `out` may alias);
//   stages     decimation in frequency, in place, one launch per stage, one
//              thread per butterfly:  lo' = a + b,  hi' = t (a - b),  t = w^(j 2^s),
//              w = omega^-1.  t = 1 skips the product (the whole last stage,
//              butterfly 0 of every block elsewhere).  The product t P uses signed
//              4-bit windows: 1P..8P of each thread go to a table in HBM, then 256
//              doublings and at most 65 additions, which every lane makes at the
//              same places whatever its twiddle.  The table-free alternative
//              (GG_ECNTT_MUL=naf, and the single product of out[0]): a left-to-right
//              double-and-add over the non-adjacent form of t, read from the bits
//              of 3t and t (digit i = bit_{i+1}(3t) - bit_{i+1}(t)), 256 doublings
//              and an addition of +-P where the digit is not 0, P read back from
//              the hi slot of the working buffer for each.
//   1/n        folded into the twiddles of block 0 of every stage: an output
//              index with lowest set bit s takes its first `hi` turn at stage s
//              in block 0, and everything downstream of that turn is linear in
//              it.  That scales every output but out[0], which one extra thread
//              multiplies at the end: log_n + 1 more products, not n.
//   normalise  batch inversion to affine (the comb's method, comb.h), writing
//              element i to out[bitrev(i)].
// xyzz_add (curve.cuh) covers infinity inputs, a = b and a = -b; the doubling
// of infinity is infinity by the formula (all coordinates 0).
#include "ecntt_impl.cuh"

namespace gg {
namespace ecntt {

template <class SC>
static void check_omega(int log_n, const void* omega_mont) {
    Fe<SC> w;
    memcpy(&w, omega_mont, sizeof(w));
    GG_CHECK(pow2k(w, log_n - 1) == -Fe<SC>::one(), GG_ERR_INVALID_ARG,
             "omega is not of exact order n = 2^" + std::to_string(log_n) + " (omega^(n/2) != -1)");
}

void check_args(int curve, int log_n, const void* omega_mont) {
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG,
             "unknown curve " + std::to_string(curve) + " (GG_CURVE_BN254 or GG_CURVE_BLS12_381)");
    GG_CHECK(log_n >= 1 && log_n <= 27, GG_ERR_INVALID_ARG,
             "log_n " + std::to_string(log_n) + " out of range (1 .. 27)");
    GG_CHECK(omega_mont, GG_ERR_INVALID_ARG, "null omega");
    if (curve == GG_CURVE_BN254) check_omega<FrCfg>(log_n, omega_mont);
    else check_omega<FrBlsCfg>(log_n, omega_mont);
}

void to_lagrange_dev(int curve, int log_n, const void* omega_mont, const void* in_dev, void* out_dev, hipStream_t st,
                     double* ms) {
    check_args(curve, log_n, omega_mont);
    if (curve == GG_CURVE_BN254)
        run<Fp, FrCfg>(log_n, omega_mont, (const Affine<Fp>*)in_dev, (Affine<Fp>*)out_dev, st, ms);
    else
        run<FpBls, FrBlsCfg>(log_n, omega_mont, (const Affine<FpBls>*)in_dev, (Affine<FpBls>*)out_dev, st, ms);
}

}  // namespace ecntt
}  // namespace gg

using namespace gg;

extern "C" int gg_kzg_to_lagrange_g1(int curve, int log_n, const void* omega_mont, const void* g1_in,
                                     int in_on_device, void* g1_out, int out_on_device, void* hip_stream) {
    GG_CAPI_BEGIN
    GG_CHECK(omega_mont && g1_in && g1_out, GG_ERR_INVALID_ARG,
             std::string("null argument: ") + (!omega_mont ? "omega_mont" : !g1_in ? "g1_in" : "g1_out"));
    ecntt::check_args(curve, log_n, omega_mont);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : hipStreamPerThread;
    ecntt::host_or_device(ecntt::point_bytes(curve) << log_n, g1_in, in_on_device, g1_out, out_on_device, st,
                          [&](const void* in, void* out) {
                              ecntt::to_lagrange_dev(curve, log_n, omega_mont, in, out, st, nullptr);
                          });
    GG_CAPI_END
}
