// PlonK Verify for batches of BLS12-381 proofs under one verifying key
// (backend/plonk/bls12-381/verify.go:45-294), and kzg.Verify for batches of
// openings: plonk_verify_impl.cuh over Bls12381Tower.  What differs from BN254
// (plonk_verify.hip):
//
//   * G1 has a cofactor.  A proof point on the curve but outside the order-r
//     subgroup is MALFORMED, as gnark's decoder rejects it: the pairing kills a
//     cofactor-order component, so ZShiftedOpening.H + T with T of small order
//     would otherwise verify as a second encoding of the same proof.  The test
//     is g1_check_endo (two multiplications by the 64-bit |x|), for the key's
//     points, the proof's and the digests and quotients of the KZG check.
//   * The point checks have lanes of their own (k_pvb_chk: one per (proof,
//     point), a flag byte each); fr_phase1 folds the 9 + n_cmt flags into the
//     status.  Chained in the per-proof lane they would be a deeper dependent
//     chain than phase 1's scalar multiplication.
//   * Every point loop (the 255-bit g1_mul, the group sums, the inversion of the
//     affine results, the subgroup test) runs over Called<FpBls>: the 12-limb
//     products are calls, each loop body stays within short-branch reach
//     (DESIGN.md "Products as calls in the r-torsion loop").
//   * RawBytes of a point is 96 B, the infinity 0x40 followed by zeros.
// Figures per kernel: DESIGN.md §4 "PlonK Verify" (its BLS12-381 part),
// profiles/r14_bls12_381_plonk_verify.md.
#include "plonk_verify_impl.cuh"

namespace gg {
namespace plonkv {

struct Bls12381 {
    using Tw = Bls12381Tower;
    using Fr = FrBls;
    using PC = Called<FpBls>;
    using P1Extra = PointFlags;
    static constexpr int kCurve = GG_CURVE_BLS12_381;
    static constexpr bool kCheckLanes = true;
    static GG_HD PC inv(const PC& a) { return PC{inv_call(a.v)}; }
    // called, so the curve equation and the endomorphism test are inlined once
    static GG_HDN int g1_flag(const Affine<FpBls>& p) { return g1_check_endo<Tw>(p); }
    static int g2_flag(const Affine<Fp2Bls>& q) { return g2_check_endo<Tw>(q); }
    // G1Affine.RawBytes of bls12-381: X | Y big-endian, the infinity 0x40 then zeros
    static void g1_raw(const Affine<FpBls>& p, uint8_t out[96]) {
        if (p.is_inf()) {
            memset(out, 0, 96);
            out[0] = 0x40;
            return;
        }
        fs::be_bytes<12>(from_mont(p.x).v, out);
        fs::be_bytes<12>(from_mont(p.y).v, out + 48);
    }
    static FrBls hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
        return pairing::hash_to_field<FrBls>(msg, len, dst, dst_len);
    }
};
using VB = Verifier<Bls12381>;
static_assert(sizeof(VB::G1P) == 96 && sizeof(VB::XZ) == 192 && VB::kLines == 68, "BLS12-381 layouts");

__global__ void __launch_bounds__(64) k_pvb_chk(VB::ChkArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.npts) VB::point_check(a, id);
}
__global__ void __launch_bounds__(256) k_pvb_pi(VB::PiArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.nslices) VB::pi_partial(a, id);
}
__global__ void __launch_bounds__(256) k_pvb_fr(VB::P1Args a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) VB::fr_phase1(a, id);
}
__global__ void __launch_bounds__(64) k_pvb_mul(VB::MulArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.T) VB::term_mul(a, id);
}
__global__ void __launch_bounds__(64) k_pvb_sum(VB::SumArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) VB::group_sum(a, id);
}
__global__ void __launch_bounds__(64) k_pvb_pair(VB::PairArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) VB::pair2(a, id);
}
template <>
struct Kernels<Bls12381> {
    static constexpr auto chk = k_pvb_chk;
    static constexpr auto pi = k_pvb_pi;
    static constexpr auto fr = k_pvb_fr;
    static constexpr auto mul = k_pvb_mul;
    static constexpr auto sum = k_pvb_sum;
    static constexpr auto pair = k_pvb_pair;
};

}  // namespace plonkv
}  // namespace gg

using namespace gg;
using VB = gg::plonkv::VB;

struct gg_plonk_vk_bls : VB::Key {};

extern "C" int gg_plonk_vk_create_bls12_381(uint64_t size, const void* generator, const void* coset_shift,
                                            const void* S, const void* Q, const void* Qcp, int n_cmt,
                                            const uint32_t* commitment_indexes, size_t nb_public,
                                            const void* kzg_g1, const void* kzg_g2, gg_plonk_vk_bls_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    std::unique_ptr<gg_plonk_vk_bls> vk(new gg_plonk_vk_bls);
    VB::create_key(vk.get(), size, generator, coset_shift, S, Q, Qcp, n_cmt, commitment_indexes, nb_public, kzg_g1,
                   kzg_g2);
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_plonk_vk_destroy_bls12_381(gg_plonk_vk_bls_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

extern "C" int gg_plonk_verify_batch_bls12_381(gg_plonk_vk_bls_t vk, size_t n, const void* proofs,
                                               const void* public_witness, gg_hash_fn challenge_hash,
                                               void* challenge_ctx, gg_hash_fn folding_hash, void* folding_ctx,
                                               uint8_t* status_out) {
    GG_CAPI_BEGIN
    VB::verify_batch(vk, true, n, proofs, public_witness, challenge_hash, challenge_ctx, folding_hash, folding_ctx,
                     status_out);
    GG_CAPI_END
}
extern "C" int gg_plonk_verify_batch_bls12_381_host(gg_plonk_vk_bls_t vk, size_t n, const void* proofs,
                                                    const void* public_witness, gg_hash_fn challenge_hash,
                                                    void* challenge_ctx, gg_hash_fn folding_hash, void* folding_ctx,
                                                    uint8_t* status_out) {
    GG_CAPI_BEGIN
    VB::verify_batch(vk, false, n, proofs, public_witness, challenge_hash, challenge_ctx, folding_hash, folding_ctx,
                     status_out);
    GG_CAPI_END
}

extern "C" int gg_kzg_verify_bls12_381(size_t n, const void* kzg_g1, const void* kzg_g2, const void* digests,
                                       const void* quotients, const void* points, const void* values,
                                       uint8_t* ok_out) {
    GG_CAPI_BEGIN
    VB::kzg_verify(true, n, kzg_g1, kzg_g2, digests, quotients, points, values, ok_out);
    GG_CAPI_END
}
extern "C" int gg_kzg_verify_bls12_381_host(size_t n, const void* kzg_g1, const void* kzg_g2, const void* digests,
                                            const void* quotients, const void* points, const void* values,
                                            uint8_t* ok_out) {
    GG_CAPI_BEGIN
    VB::kzg_verify(false, n, kzg_g1, kzg_g2, digests, quotients, points, values, ok_out);
    GG_CAPI_END
}
