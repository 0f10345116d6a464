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

}  // namespace pairing
}  // namespace gg
