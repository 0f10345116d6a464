// PlonK Verify for batches of BN254 proofs under one verifying key
// (backend/plonk/bn254/verify.go:45-294), and the plain KZG opening check it
// is made of (kzg.Verify): plonk_verify_impl.cuh over Bn254Tower.  The steps,
// the batch driver and the KZG driver are the header's; this file holds the
// curve's traits, the five kernels and the C entry points.  The point checks are
// the curve equation (cofactor 1), chained in fr_phase1; the point loops run
// over Fp with the products inlined.  BLS12-381: plonk_verify_bls.hip.
#include "plonk_verify_impl.cuh"

namespace gg {
namespace plonkv {

struct Bn254 {
    using Tw = Bn254Tower;
    using Fr = gg::Fr;
    using PC = Fp;
    using P1Extra = NoFlags;
    static constexpr int kCurve = GG_CURVE_BN254;
    static constexpr bool kCheckLanes = false;
    static GG_HD Fp inv(const Fp& a) { return inverse(a); }
    static GG_HD int g1_flag(const G1Affine& p) { return g1_check<Tw>(p); }
    static int g2_flag(const G2Affine& q) { return g2_check<Tw>(q); }
    // G1Affine.RawBytes = Marshal of bn254: X | Y big-endian, the infinity all zeros
    static void g1_raw(const G1Affine& p, uint8_t out[64]) {
        fs::be_bytes<8>(from_mont(p.x).v, out);
        fs::be_bytes<8>(from_mont(p.y).v, out + 32);
    }
    static gg::Fr hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
        return pairing::hash_to_field<gg::Fr>(msg, len, dst, dst_len);
    }
};
using V = Verifier<Bn254>;

__global__ void __launch_bounds__(256) k_pv_pi(V::PiArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.nslices) V::pi_partial(a, id);
}
__global__ void __launch_bounds__(256) k_pv_fr(V::P1Args a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) V::fr_phase1(a, id);
}
__global__ void __launch_bounds__(64) k_pv_mul(V::MulArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n * a.T) V::term_mul(a, id);
}
__global__ void __launch_bounds__(64) k_pv_sum(V::SumArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) V::group_sum(a, id);
}
__global__ void __launch_bounds__(64) k_pv_pair(V::PairArgs a) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < a.n) V::pair2(a, id);
}
template <>
struct Kernels<Bn254> {
    static constexpr auto pi = k_pv_pi;
    static constexpr auto fr = k_pv_fr;
    static constexpr auto mul = k_pv_mul;
    static constexpr auto sum = k_pv_sum;
    static constexpr auto pair = k_pv_pair;
};

}  // namespace plonkv
}  // namespace gg

using namespace gg;
using V = gg::plonkv::V;

struct gg_plonk_vk : V::Key {};

extern "C" int gg_plonk_vk_create(int curve, uint64_t size, const void* generator, const void* coset_shift,
                                  const void* S, const void* Q, const void* Qcp, int n_cmt,
                                  const uint32_t* commitment_indexes, size_t nb_public, const void* kzg_g1,
                                  const void* kzg_g2, gg_plonk_vk_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    GG_CHECK(curve == GG_CURVE_BN254, GG_ERR_UNSUPPORTED,
             "curve " + std::to_string(curve) +
                 " is not supported: this entry point is BN254's (BLS12-381: gg_plonk_vk_create_bls12_381)");
    std::unique_ptr<gg_plonk_vk> vk(new gg_plonk_vk);
    V::create_key(vk.get(), size, generator, coset_shift, S, Q, Qcp, n_cmt, commitment_indexes, nb_public, kzg_g1,
                  kzg_g2);
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_plonk_vk_destroy(gg_plonk_vk_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

extern "C" int gg_plonk_verify_batch(gg_plonk_vk_t vk, size_t n, const void* proofs, const void* public_witness,
                                     gg_hash_fn challenge_hash, void* challenge_ctx, gg_hash_fn folding_hash,
                                     void* folding_ctx, uint8_t* status_out) {
    GG_CAPI_BEGIN
    V::verify_batch(vk, true, n, proofs, public_witness, challenge_hash, challenge_ctx, folding_hash, folding_ctx,
                    status_out);
    GG_CAPI_END
}
extern "C" int gg_plonk_verify_batch_host(gg_plonk_vk_t vk, size_t n, const void* proofs, const void* public_witness,
                                          gg_hash_fn challenge_hash, void* challenge_ctx, gg_hash_fn folding_hash,
                                          void* folding_ctx, uint8_t* status_out) {
    GG_CAPI_BEGIN
    V::verify_batch(vk, false, n, proofs, public_witness, challenge_hash, challenge_ctx, folding_hash, folding_ctx,
                    status_out);
    GG_CAPI_END
}

extern "C" int gg_kzg_verify_bn254(size_t n, const void* kzg_g1, const void* kzg_g2, const void* digests,
                                   const void* quotients, const void* points, const void* values, uint8_t* ok_out) {
    GG_CAPI_BEGIN
    V::kzg_verify(true, n, kzg_g1, kzg_g2, digests, quotients, points, values, ok_out);
    GG_CAPI_END
}
extern "C" int gg_kzg_verify_bn254_host(size_t n, const void* kzg_g1, const void* kzg_g2, const void* digests,
                                        const void* quotients, const void* points, const void* values,
                                        uint8_t* ok_out) {
    GG_CAPI_BEGIN
    V::kzg_verify(false, n, kzg_g1, kzg_g2, digests, quotients, points, values, ok_out);
    GG_CAPI_END
}
