// EC-NTT over G2: the templates of ecntt_impl.cuh over the twist's coordinate
// field, for [tau^j]2 -> [L_i(tau)]2 (the pk.G2.B side of a Groth16 key made from
// a powers-of-tau SRS, backend/groth16/bn254/mpcsetup/phase2.go:71 and
// lagrange.go:25-40).  The contract of gg_kzg_to_lagrange_g1, argument for
// argument.
//
// BN254 runs over Fp2 with its products inlined, as the G1 kernels do.  Over
// BLS12-381 every kernel runs over Called<Fp2Bls> (pairing.cuh: the same bytes,
// the 12-limb Karatsuba product and the squaring as real calls): the window
// multiplication's loop body is four doublings and an addition, 80 Fp2Bls
// products, which inlined is far past short-branch reach (DESIGN.md §4
// "Products as calls in the r-torsion loop").
#include "ecntt_impl.cuh"
#include "pairing.cuh"

namespace gg {
namespace ecntt {

using G2Bls = pairing::Called<Fp2Bls>;
static_assert(sizeof(Affine<G2Bls>) == 192 && sizeof(Xyzz<G2Bls>) == 384, "Called<> adds no bytes");

void to_lagrange_g2_dev(int curve, int log_n, const void* omega_mont, const void* in_dev, void* out_dev,
                        hipStream_t st, double* ms) {
    check_args(curve, log_n, omega_mont);
    if (curve == GG_CURVE_BN254)
        run<Fp2, FrCfg>(log_n, omega_mont, (const Affine<Fp2>*)in_dev, (Affine<Fp2>*)out_dev, st, ms);
    else
        run<G2Bls, FrBlsCfg>(log_n, omega_mont, (const Affine<G2Bls>*)in_dev, (Affine<G2Bls>*)out_dev, st, ms);
}

}  // namespace ecntt
}  // namespace gg

using namespace gg;

extern "C" int gg_kzg_to_lagrange_g2(int curve, int log_n, const void* omega_mont, const void* g2_in,
                                     int in_on_device, void* g2_out, int out_on_device, void* hip_stream) {
    GG_CAPI_BEGIN
    GG_CHECK(omega_mont && g2_in && g2_out, GG_ERR_INVALID_ARG,
             std::string("null argument: ") + (!omega_mont ? "omega_mont" : !g2_in ? "g2_in" : "g2_out"));
    ecntt::check_args(curve, log_n, omega_mont);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : hipStreamPerThread;
    ecntt::host_or_device(ecntt::point_bytes_g2(curve) << log_n, g2_in, in_on_device, g2_out, out_on_device, st,
                          [&](const void* in, void* out) {
                              ecntt::to_lagrange_g2_dev(curve, log_n, omega_mont, in, out, st, nullptr);
                          });
    GG_CAPI_END
}
