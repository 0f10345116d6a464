// gnark-crypto's point codec over BN254: point_codec_impl.cuh over Bn254Tower
// (2-bit flags, 32-byte coordinates; G1 has no cofactor, G2 gets the
// multiplication by r behind gg_g2_check_bn254), and the C entry points of both
// curves (BLS12-381: point_codec_bls.hip).
// Every argument is validated on the host before the first device call.
#include "point_codec_impl.cuh"

namespace gg {
namespace codec {

struct Bn254 {
    using Tw = Bn254Tower;
    static constexpr bool ZCASH = false;
    static GG_HD bool g1_member(const Affine<Fp>&) { return true; }
    static GG_HD bool g2_member(const Affine<Fp2>& q) { return times_r_is_inf<Tw, Fp2>(q); }
};
static_assert(Codec<Bn254>::encoded_size(false, GG_ENC_COMPRESSED) == 32 &&
                  Codec<Bn254>::encoded_size(true, GG_ENC_RAW) == 128,
              "BN254 encoded sizes");

GG_CODEC_KERNELS(Bn254, k_codec)

static bool group_ok(int group) {
    return group == GG_G1 || group == GG_G2 || group == GG_BLS12_381_G1 || group == GG_BLS12_381_G2;
}
static bool is_bls(int group) { return group == GG_BLS12_381_G1 || group == GG_BLS12_381_G2; }
static bool is_g2(int group) { return group == GG_G2 || group == GG_BLS12_381_G2; }

static void check_common(int group, int enc, size_t n) {
    GG_CHECK(group_ok(group), GG_ERR_INVALID_ARG,
             "group must be GG_G1, GG_G2, GG_BLS12_381_G1 or GG_BLS12_381_G2, got " + std::to_string(group));
    GG_CHECK(enc == GG_ENC_COMPRESSED || enc == GG_ENC_RAW, GG_ERR_INVALID_ARG,
             "enc must be GG_ENC_COMPRESSED or GG_ENC_RAW, got " + std::to_string(enc));
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(n <= ((size_t)1 << 32), GG_ERR_INVALID_ARG, "n exceeds 2^32 points per call");
}
static void decode(bool dev, int group, int enc, int flags, size_t n, const void* bytes, bool bytes_on_device,
                   void* points_out, bool out_on_device, uint8_t* status_out) {
    check_common(group, enc, n);
    GG_CHECK((flags & ~GG_DEC_NO_SUBGROUP_CHECK) == 0, GG_ERR_INVALID_ARG,
             "flags must be 0 or GG_DEC_NO_SUBGROUP_CHECK, got " + std::to_string(flags));
    GG_CHECK(bytes, GG_ERR_INVALID_ARG, "null argument: bytes");
    GG_CHECK(points_out, GG_ERR_INVALID_ARG, "null argument: points_out");
    GG_CHECK(status_out, GG_ERR_INVALID_ARG, "null argument: status_out");
    if (is_bls(group))
        bls_decode(dev, is_g2(group), enc, flags, n, bytes, bytes_on_device, points_out, out_on_device, status_out);
    else
        Api<Bn254>::decode(dev, is_g2(group), enc, flags, n, bytes, bytes_on_device, points_out, out_on_device,
                           status_out);
}
static void encode(bool dev, int group, int enc, size_t n, const void* points, bool points_on_device,
                   void* bytes_out) {
    check_common(group, enc, n);
    GG_CHECK(points, GG_ERR_INVALID_ARG, "null argument: points");
    GG_CHECK(bytes_out, GG_ERR_INVALID_ARG, "null argument: bytes_out");
    if (is_bls(group)) bls_encode(dev, is_g2(group), enc, n, points, points_on_device, bytes_out);
    else Api<Bn254>::encode(dev, is_g2(group), enc, n, points, points_on_device, bytes_out);
}
static void fp_sqrt_entry(bool dev, int curve, int degree, size_t n, const void* in, void* out, uint8_t* ok) {
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG,
             "curve must be GG_CURVE_BN254 or GG_CURVE_BLS12_381, got " + std::to_string(curve));
    GG_CHECK(degree == 1 || degree == 2, GG_ERR_INVALID_ARG, "degree must be 1 (Fp) or 2 (Fp2)");
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(n <= ((size_t)1 << 32), GG_ERR_INVALID_ARG, "n exceeds 2^32 elements per call");
    GG_CHECK(in, GG_ERR_INVALID_ARG, "null argument: in_mont");
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out_mont");
    GG_CHECK(ok, GG_ERR_INVALID_ARG, "null argument: ok_out");
    if (curve == GG_CURVE_BLS12_381) bls_sqrt(dev, degree, n, in, out, ok);
    else Api<Bn254>::sqrt(dev, degree, n, in, out, ok);
}

}  // namespace codec
}  // namespace gg

using namespace gg;

extern "C" size_t gg_point_encoded_size(int group, int enc) {
    if (!codec::group_ok(group) || (enc != GG_ENC_COMPRESSED && enc != GG_ENC_RAW)) return 0;
    return (size_t)(codec::is_bls(group) ? 48 : 32) * (codec::is_g2(group) ? 2 : 1) * (enc == GG_ENC_RAW ? 2 : 1);
}
extern "C" int gg_points_decode(int group, int enc, int flags, size_t n, const void* bytes, int bytes_on_device,
                                void* points_out, int out_on_device, uint8_t* status_out) {
    GG_CAPI_BEGIN
    codec::decode(true, group, enc, flags, n, bytes, bytes_on_device != 0, points_out, out_on_device != 0,
                  status_out);
    GG_CAPI_END
}
extern "C" int gg_points_decode_host(int group, int enc, int flags, size_t n, const void* bytes, void* points_out,
                                     uint8_t* status_out) {
    GG_CAPI_BEGIN
    codec::decode(false, group, enc, flags, n, bytes, false, points_out, false, status_out);
    GG_CAPI_END
}
extern "C" int gg_points_encode(int group, int enc, size_t n, const void* points, int points_on_device,
                                void* bytes_out) {
    GG_CAPI_BEGIN
    codec::encode(true, group, enc, n, points, points_on_device != 0, bytes_out);
    GG_CAPI_END
}
extern "C" int gg_points_encode_host(int group, int enc, size_t n, const void* points, void* bytes_out) {
    GG_CAPI_BEGIN
    codec::encode(false, group, enc, n, points, false, bytes_out);
    GG_CAPI_END
}
extern "C" int gg_fp_sqrt(int curve, int degree, size_t n, const void* in_mont, void* out_mont, uint8_t* ok_out) {
    GG_CAPI_BEGIN
    codec::fp_sqrt_entry(true, curve, degree, n, in_mont, out_mont, ok_out);
    GG_CAPI_END
}
extern "C" int gg_fp_sqrt_host(int curve, int degree, size_t n, const void* in_mont, void* out_mont,
                               uint8_t* ok_out) {
    GG_CAPI_BEGIN
    codec::fp_sqrt_entry(false, curve, degree, n, in_mont, out_mont, ok_out);
    GG_CAPI_END
}
