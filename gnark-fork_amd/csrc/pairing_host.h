// Host helpers that the pairing entry points (pairing.hip), the Groth16 verifier
// (groth16_verify_impl.cuh) and the PlonK verifier (plonk_verify_impl.cuh) share.
#pragma once
#include "field.cuh"
#include <cstddef>
#include <cstdint>

namespace gg {
namespace pairing {

// RFC 9380 5.3.1 expand_message_xmd over SHA-256: the first 48 bytes in out (dst_len <= 255)
void expand_message_xmd48(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint8_t out[64]);

// big-endian bytes mod r, Montgomery form (Horner over the bytes)
template <class F>
inline F fr_from_be(const uint8_t* b, size_t n) {
    F m256 = F::zero(), acc = F::zero();
    m256.v[0] = 256;
    m256 = to_mont(m256);
    for (size_t i = 0; i < n; i++) {
        F d = F::zero();
        d.v[0] = b[i];
        acc = acc * m256 + to_mont(d);
    }
    return acc;
}
// fr.Hash(msg, dst, 1): expand_message_xmd over SHA-256, 48 bytes, big-endian,
// mod r; Montgomery form
template <class F>
inline F hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
    uint8_t out[64];
    expand_message_xmd48(msg, len, dst, dst_len, out);
    return fr_from_be<F>(out, 48);
}

}  // namespace pairing
}  // namespace gg
