// Groth16 Verify over BLS12-381 for batches of proofs under one verifying key
// (backend/groth16/bls12-381/verify.go:42-140): groth16_verify_impl.cuh over
// Bls12381Tower, and the endomorphism membership checks it introduces.  What
// differs from BN254 (groth16_verify.hip):
//
//   * G1 has a cofactor: Ar, Krs, every commitment and the PoK get a subgroup
//     test as Bs does.  The tests are g1_check_endo / g2_check_endo, both
//     measured faster than the multiplication by r
//     (profiles/r13_bls12_381_groth16_verify.md).
//   * Every point loop runs over Called<FpBls> (pairing.cuh: the 12-limb products
//     as real calls), so no loop body grows past short-branch reach.
//   * The key is created on the host alone; the first device batch uploads it
//     and builds the table.  gg_groth16_verify_batch_bls12_381_host runs the
//     per-proof functions in a loop on the calling thread, with no device call.
// Figures per kernel: DESIGN.md §4 "Groth16 Verify",
// profiles/groth16_verify_refactor.md.
#include "groth16_verify_impl.cuh"
#include <memory>

namespace gg {
namespace groth16v {

struct Bls12381 {
    using Tw = Bls12381Tower;
    using Fr = FrBls;
    using PC = Called<FpBls>;
    static constexpr unsigned kPubBlock = 64;
    static GG_HD PC inv(const PC& a) { return PC{inv_call(a.v)}; }
    // called, so the curve equation and the endomorphism test are inlined once
    static GG_HDN int g1_flag(const Affine<FpBls>& p) { return g1_check_endo<Tw>(p); }
    static GG_HDN int g2_flag(const Affine<Fp2Bls>& q) { return g2_check_endo<Tw>(q); }
};
using VB = Verifier<Bls12381>;
static_assert(sizeof(VB::Proof) == 384 && sizeof(VB::XZ) == 192 && VB::kLines == 68, "BLS12-381 layouts");

__global__ void __launch_bounds__(64) k_g16b_table(VB::TableArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.nsc * 32) VB::table_lane(a, id);
}
__global__ void __launch_bounds__(64) k_g16b_pub_partial(VB::PubArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.nslices) VB::pub_partial_one(a, id);
}
__global__ void __launch_bounds__(64) k_g16b_prep(VB::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) VB::prep_one(a, i);
}
__global__ void __launch_bounds__(64) k_g16b_pair(VB::Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) VB::pair_one(a, i);
}
template <>
struct Kernels<Bls12381> {
    static constexpr auto table = k_g16b_table;
    static constexpr auto pub = k_g16b_pub_partial;
    static constexpr auto prep = k_g16b_prep;
    static constexpr auto pair = k_g16b_pair;
};

__global__ void __launch_bounds__(64) k_g1_check_endo_bls(size_t n, const VB::G1A* p, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g1_check_endo<Bls12381Tower>(p[i]);
}
__global__ void __launch_bounds__(64) k_g2_check_endo_bls(size_t n, const VB::G2A* q, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g2_check_endo<Bls12381Tower>(q[i]);
}

}  // namespace groth16v
}  // namespace gg

using namespace gg;
using namespace gg::groth16v;

struct gg_groth16_vk_bls : VB::Key {};

extern "C" int gg_groth16_vk_create_bls12_381(const void* alpha1, const void* beta2, const void* gamma2,
                                              const void* delta2, const void* K, size_t n_K, size_t nb_public,
                                              const void* ped_g, const void* ped_g_root_sigma_neg,
                                              const uint32_t* committed_off, const uint32_t* committed_idx,
                                              int n_commitments, gg_groth16_vk_bls_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    std::unique_ptr<gg_groth16_vk_bls> vk(new gg_groth16_vk_bls);
    VB::create_key(vk.get(), alpha1, beta2, gamma2, delta2, K, n_K, nb_public, ped_g, ped_g_root_sigma_neg,
                   committed_off, committed_idx, n_commitments);
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_groth16_vk_destroy_bls12_381(gg_groth16_vk_bls_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

extern "C" int gg_groth16_verify_batch_bls12_381(gg_groth16_vk_bls_t vk, size_t n, const void* proofs,
                                                 const void* commitments, const void* poks,
                                                 const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    VB::verify_batch(vk, true, n, proofs, commitments, poks, public_witness, status_out);
    GG_CAPI_END
}
extern "C" int gg_groth16_verify_batch_bls12_381_host(gg_groth16_vk_bls_t vk, size_t n, const void* proofs,
                                                      const void* commitments, const void* poks,
                                                      const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    VB::verify_batch(vk, false, n, proofs, commitments, poks, public_witness, status_out);
    GG_CAPI_END
}

extern "C" int gg_hash_to_field_bls12_381(const void* msg, size_t len, const void* dst, size_t dst_len, void* out32) {
    GG_CAPI_BEGIN
    GG_CHECK(msg || !len, GG_ERR_INVALID_ARG, "null argument: msg");
    GG_CHECK(dst || !dst_len, GG_ERR_INVALID_ARG, "null argument: dst");
    GG_CHECK(out32, GG_ERR_INVALID_ARG, "null argument: out32");
    GG_CHECK(dst_len <= 255, GG_ERR_INVALID_ARG, "dst_len must be <= 255 (expand_message_xmd)");
    const FrBls h = hash_to_field<FrBls>((const uint8_t*)msg, len, (const uint8_t*)dst, dst_len);
    memcpy(out32, &h, 32);
    GG_CAPI_END
}
extern "C" int gg_g1_check_endo_bls12_381(size_t n, const void* g1, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g1, "g1", flags_out);
    run_check<VB::G1A>(n, g1, flags_out, k_g1_check_endo_bls, 64);
    GG_CAPI_END
}
extern "C" int gg_g2_check_endo_bls12_381(size_t n, const void* g2, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g2, "g2", flags_out);
    run_check<VB::G2A>(n, g2, flags_out, k_g2_check_endo_bls, 64);
    GG_CAPI_END
}
