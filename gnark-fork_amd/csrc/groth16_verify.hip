// Groth16 Verify for batches of BN254 proofs under one verifying key
// (backend/groth16/bn254/verify.go:43-140): groth16_verify_impl.cuh over
// Bn254Tower.  The steps and the batch driver are the header's; this file holds
// the curve's traits, the four kernels and the C entry points.  The point checks
// are g1_check / g2_check (G1 has cofactor 1); the point loops run over Fp with
// the products inlined.  The key is uploaded, and bound to the current device,
// when it is created.  BLS12-381: groth16_verify_bls.hip.  Figures per kernel:
// DESIGN.md §4 "Groth16 Verify", profiles/groth16_verify_refactor.md.
#include "groth16_verify_impl.cuh"
#include <memory>

namespace gg {
namespace groth16v {

struct Bn254 {
    using Tw = Bn254Tower;
    using Fr = gg::Fr;
    using PC = Fp;
    static constexpr unsigned kPubBlock = 256;
    static GG_HD Fp inv(const Fp& a) { return inverse(a); }
    static GG_HD int g1_flag(const G1Affine& p) { return g1_check<Tw>(p); }
    static GG_HD int g2_flag(const G2Affine& q) { return g2_check<Tw>(q); }
};
using V = Verifier<Bn254>;
static_assert(sizeof(V::Proof) == 256 && sizeof(V::LineT) == 192, "BN254 layouts");

__global__ void __launch_bounds__(64) k_vk_table(V::TableArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.nsc * 32) V::table_lane(a, id);
}
__global__ void __launch_bounds__(256) k_pub_partial(V::PubArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.nslices) V::pub_partial_one(a, id);
}
__global__ void __launch_bounds__(64) k_g16_prep(V::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) V::prep_one(a, i);
}
__global__ void __launch_bounds__(64) k_g16_pair(V::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) V::pair_one(a, i);
}
template <>
struct Kernels<Bn254> {
    static constexpr auto table = k_vk_table;
    static constexpr auto pub = k_pub_partial;
    static constexpr auto prep = k_g16_prep;
    static constexpr auto pair = k_g16_pair;
};

}  // namespace groth16v
}  // namespace gg

using namespace gg;
using V = gg::groth16v::V;

struct gg_groth16_vk : V::Key {};

extern "C" int gg_groth16_vk_create(int curve, const void* alpha1, const void* beta2, const void* gamma2,
                                    const void* delta2, const void* K, size_t n_K, size_t nb_public,
                                    const void* ped_g, const void* ped_g_root_sigma_neg,
                                    const uint32_t* committed_off, const uint32_t* committed_idx, int n_commitments,
                                    gg_groth16_vk_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    GG_CHECK(curve == GG_CURVE_BN254, GG_ERR_UNSUPPORTED,
             "curve " + std::to_string(curve) + " is not supported: Groth16 Verify has a BN254 pairing only");
    std::unique_ptr<gg_groth16_vk> vk(new gg_groth16_vk);
    V::create_key(vk.get(), alpha1, beta2, gamma2, delta2, K, n_K, nb_public, ped_g, ped_g_root_sigma_neg,
                  committed_off, committed_idx, n_commitments);
    V::upload_key(vk.get());
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_groth16_vk_destroy(gg_groth16_vk_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

extern "C" int gg_groth16_verify_batch(gg_groth16_vk_t vk, size_t n, const void* proofs, const void* commitments,
                                       const void* poks, const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    V::verify_batch(vk, true, n, proofs, commitments, poks, public_witness, status_out);
    GG_CAPI_END
}
