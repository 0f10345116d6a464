// gnark-crypto's point codec over BLS12-381: point_codec_impl.cuh over
// Bls12381Tower.  The Zcash flag layout (3 bits), 48-byte coordinates, and the
// endomorphism membership tests of the verifiers (pairing.cuh: g1_endo_is_member,
// g2_endo_is_member) on both groups, since G1 has a cofactor here.
#include "point_codec_impl.cuh"

namespace gg {
namespace codec {

struct Bls12381 {
    using Tw = Bls12381Tower;
    static constexpr bool ZCASH = true;
    static GG_HD bool g1_member(const Affine<FpBls>& p) { return g1_endo_is_member<Tw>(p); }
    static GG_HD bool g2_member(const Affine<Fp2Bls>& q) { return g2_endo_is_member<Tw>(q); }
};
static_assert(Codec<Bls12381>::encoded_size(false, GG_ENC_COMPRESSED) == 48 &&
                  Codec<Bls12381>::encoded_size(true, GG_ENC_RAW) == 192,
              "BLS12-381 encoded sizes");

GG_CODEC_KERNELS(Bls12381, k_codec_bls)

void bls_decode(bool dev, bool g2, int enc, int flags, size_t n, const void* bytes, bool bytes_on_device,
                void* points_out, bool out_on_device, uint8_t* status_out) {
    Api<Bls12381>::decode(dev, g2, enc, flags, n, bytes, bytes_on_device, points_out, out_on_device, status_out);
}
void bls_encode(bool dev, bool g2, int enc, size_t n, const void* points, bool points_on_device, void* bytes_out) {
    Api<Bls12381>::encode(dev, g2, enc, n, points, points_on_device, bytes_out);
}
void bls_sqrt(bool dev, int degree, size_t n, const void* in, void* out, uint8_t* ok) {
    Api<Bls12381>::sqrt(dev, degree, n, in, out, ok);
}

}  // namespace codec
}  // namespace gg
