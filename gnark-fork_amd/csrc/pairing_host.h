// Host helpers of pairing.hip that the PlonK verifier (plonk_verify.hip) shares.
#pragma once
#include "field.cuh"
#include <cstddef>
#include <cstdint>

namespace gg {
namespace pairing {

// RFC 9380 5.3.1 expand_message_xmd over SHA-256: the first 48 bytes in out (dst_len <= 255)
void expand_message_xmd48(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint8_t out[64]);
// fr.Hash(msg, dst, 1): RFC 9380 expand_message_xmd over SHA-256, 48 bytes,
// big-endian, mod r; Montgomery form
Fr hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len);

// The same over the BLS12-381 scalar field, shared by the Groth16 and the PlonK
// verifier of that curve.
// big-endian bytes mod r, Montgomery form (Horner over the bytes)
inline FrBls frb_from_be(const uint8_t* b, size_t n) {
    FrBls m256 = FrBls::zero(), acc = FrBls::zero();
    m256.v[0] = 256;
    m256 = to_mont(m256);
    for (size_t i = 0; i < n; i++) {
        FrBls d = FrBls::zero();
        d.v[0] = b[i];
        acc = acc * m256 + to_mont(d);
    }
    return acc;
}
inline FrBls hash_to_field_bls(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
    uint8_t out[64];
    expand_message_xmd48(msg, len, dst, dst_len, out);
    return frb_from_be(out, 48);
}

}  // namespace pairing
}  // namespace gg
