// Groth16 Verify over BLS12-381 for batches of proofs under one verifying key
// (backend/groth16/bls12-381/verify.go:42-140), BSB22 commitments included, and
// the endomorphism membership checks it introduces.
//
// Shape: the one of the BN254 verifier (pairing.hip), over Bls12381Tower.  One
// lane per proof, 64-lane blocks; the Fp12 / Fp6 routines are real calls and
// their operands live in the lane's stack frame.  Every point loop runs over
// Called<FpBls> (pairing.cuh: the 12-limb products as real calls), so no loop
// body grows past short-branch reach.  Figures per kernel: DESIGN.md §4
// "Groth16 Verify, BLS12-381", profiles/r13_bls12_381_groth16_verify.md.
//
//   k_g16b_table        T[t][w][j] = j 2^(8w) K[t + 1]: a lane builds its 256
//                       multiples (XYZZ) and normalises them with one inversion
//   k_g16b_pub_partial  one lane per (proof, slice of 8 public inputs): 32 mixed
//                       additions per scalar, no doubling; exact for 0 and r - 1
//   k_g16b_prep         per proof: the point checks, kSum, the folded commitment
//   k_g16b_pair         per proof: the Pedersen check, then the 3-pair Miller loop
//                       with the key's line tables for -delta and -gamma, the
//                       final exponentiation and the comparison with e(alpha, beta)^3
//   k_g1_check_endo_bls / k_g2_check_endo_bls   the endomorphism checks alone
// The bodies of prep and pair are GG_HD functions (g16_prep_one, g16_pair_one):
// gg_groth16_verify_batch_bls12_381_host runs them in a loop on the calling
// thread, with the public-input sum by plain scalar multiplication.
// The key is created on the host alone; the first device batch uploads it and
// builds the table.  The commitment hashes and the folding challenge run on the
// host.  Every argument is validated before the first device call.
#include "common.h"
#include "pairing.cuh"
#include "pairing_host.h"
#include "pairing_run.h"
#include "sha256.h"
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace gg {
namespace pairing {

using TwB = Bls12381Tower;
using GTB = Fp12<TwB>;
using LineB = Line<TwB>;
using G1B = Affine<FpBls>;
using G2B = Affine<Fp2Bls>;
using CF = Called<FpBls>;  // FpBls with its products as calls; the same bytes
using G1C = Affine<CF>;
using XyzzC = Xyzz<CF>;
using JacC = Jac<CF>;
constexpr int kLinesB = line_count<TwB>();
constexpr int kSliceB = 8;  // public inputs per lane of k_g16b_pub_partial
static_assert(sizeof(G1C) == sizeof(G1B) && sizeof(XyzzC) == 4 * sizeof(FpBls), "Called<> adds no bytes");
static_assert(kLinesB == 68, "63 doublings + 5 additions");

struct ProofB {
    G1B ar;
    G2B bs;
    G1B krs;
};
static_assert(sizeof(ProofB) == 384, "proof layout");

GG_HD G1C to_c(const G1B& a) { return G1C{CF{a.x}, CF{a.y}}; }

GG_HDN G1B xyzz_to_affine_c(const XyzzC& p) {
    if (p.is_inf()) return G1B::inf();
    const CF i3{inv_call(p.zzz.v)};
    return G1B{(p.x * sqr(p.zz * i3)).v, (p.y * i3).v};
}
GG_HDN G1B jac_to_affine_c(const JacC& p) {
    if (p.is_inf()) return G1B::inf();
    const CF zi{inv_call(p.z.v)};
    const CF zi2 = sqr(zi);
    return G1B{(p.x * zi2).v, (p.y * zi2 * zi).v};
}
// k a for a canonical scalar of 8 words
GG_HDN JacC g1_mul_words_c(const JacC& a, const uint32_t* k) {
    JacC acc = JacC::inf();
    for (int wd = 7; wd >= 0; wd--) {
        const uint32_t word = k[wd];
        for (int b = 31; b >= 0; b--) {
            acc = jac_dbl(acc);
            if ((word >> b) & 1) acc = jac_add(acc, a);
        }
    }
    return acc;
}
// the verifier's flags (0 good, 1 off the curve, 2 outside the subgroup) by the
// endomorphism checks, both measured faster than the multiplication by r
// (profiles/r13_bls12_381_groth16_verify.md); called, so the curve equation is inlined once
GG_HDN int g1_flag(const G1B& p) { return g1_check_endo<TwB>(p); }
GG_HDN int g2_flag(const G2B& q) { return g2_check_endo<TwB>(q); }

// what the per-proof functions read and write: the batch, the key, the work arrays
struct G16Args {
    size_t n, nc, nslices;
    const ProofB* proofs;
    const G1B *cmts, *poks, *K;
    const XyzzC* part;     // n x nslices partial public-input sums
    const uint32_t* chal;  // n x 8 words: the folding challenge, canonical (nc > 1)
    G1B *ksum, *folded;
    uint8_t* status;
    const LineB *delta_neg, *gamma_neg, *ped_g, *ped_gs;
    const GTB* e;
};

// proof.isValid (verify.go:61), kSum (110-119) and the folded commitment
GG_HD void g16_prep_one(const G16Args& a, size_t i) {
    const ProofB& pr = a.proofs[i];
    const size_t nc = a.nc;
    bool bad = g1_flag(pr.ar) != 0;
    if (!bad) bad = g1_flag(pr.krs) != 0;
    for (size_t j = 0; j < nc && !bad; j++) bad = g1_flag(a.cmts[i * nc + j]) != 0;
    if (nc && !bad) bad = g1_flag(a.poks[i]) != 0;
    if (!bad) bad = g2_flag(pr.bs) != 0;
    if (bad) {
        a.status[i] = GG_VERIFY_SUBGROUP;
        return;
    }
    XyzzC acc = XyzzC::from_affine(to_c(a.K[0]));
    for (size_t s = 0; s < a.nslices; s++) xyzz_add_inplace(acc, a.part[i * a.nslices + s]);
    for (size_t j = 0; j < nc; j++) {
        const G1C c = to_c(a.cmts[i * nc + j]);
        if (!c.is_inf()) xyzz_madd_inplace(acc, c);
    }
    a.ksum[i] = xyzz_to_affine_c(acc);
    if (nc) {  // sum_j r^j C_j by Horner (pedersen.FoldCommitments; one commitment: itself)
        JacC f = JacC::from_affine(to_c(a.cmts[i * nc + nc - 1]));
        for (size_t j = nc - 1; j-- > 0;)
            f = jac_add(g1_mul_words_c(f, a.chal + 8 * i), JacC::from_affine(to_c(a.cmts[i * nc + j])));
        a.folded[i] = jac_to_affine_c(f);
    }
    a.status[i] = GG_VERIFY_OK;
}

// the Pedersen check (verify.go:105), then the pairing equation (124-135)
GG_HD void g16_pair_one(const G16Args& a, size_t i) {
    if (a.status[i] != GG_VERIFY_OK) return;
    G1B p[3];
    G2Src<TwB> s[3];
    if (a.nc) {  // e(folded, G) e(pok, GRootSigmaNeg) == 1
        p[0] = a.folded[i];
        p[1] = a.poks[i];
        s[0].tab = a.ped_g;
        s[0].skip = p[0].is_inf();
        s[1].tab = a.ped_gs;
        s[1].skip = p[1].is_inf();
        GTB f = GTB::one();
        miller_loop<TwB, 2>(f, p, s);
        if (!final_exp(f).is_one()) {
            a.status[i] = GG_VERIFY_PEDERSEN;
            return;
        }
    }
    const ProofB& pr = a.proofs[i];
    p[0] = pr.krs;
    p[1] = pr.ar;
    p[2] = a.ksum[i];
    s[0].tab = a.delta_neg;
    s[0].pos = 0;
    s[0].skip = p[0].is_inf();
    src_init<TwB>(s[1], pr.bs, nullptr, p[1].is_inf());
    s[2].tab = a.gamma_neg;
    s[2].pos = 0;
    s[2].skip = p[2].is_inf();
    GTB f = GTB::one();
    miller_loop<TwB, 3>(f, p, s);
    a.status[i] = final_exp(f) == *a.e ? GG_VERIFY_OK : GG_VERIFY_PAIRING;
}

__global__ void __launch_bounds__(64) k_g16b_prep(G16Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) g16_prep_one(a, i);
}
__global__ void __launch_bounds__(64) k_g16b_pair(G16Args a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) g16_pair_one(a, i);
}

// lane (t, w): the 256 multiples of 2^(8w) K[t + 1], XYZZ in cur, affine in out.
// The lane normalises its own 256 points with one inversion; the prefix
// products wait in the x coordinate of the output slot they belong to.
__global__ void __launch_bounds__(64) k_g16b_table(const G1B* K, size_t nsc, XyzzC* cur, G1B* out) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nsc * 32) return;
    const size_t t = id >> 5;
    const int w = (int)(id & 31);
    XyzzC b = XyzzC::from_affine(to_c(K[t + 1]));
    for (int s = 0; s < 8 * w; s++) b = xyzz_dbl(b);
    XyzzC* o = cur + id * 256;
    G1B* r = out + id * 256;
    XyzzC acc = b;
    CF prod = CF::one();
    r[0] = G1B::inf();
    for (int j = 1; j < 256; j++) {
        o[j] = acc;
        r[j].x = prod.v;
        if (!acc.is_inf()) prod = prod * acc.zzz;
        acc = xyzz_add(acc, b);
    }
    CF inv{inv_call(prod.v)};
    for (int j = 255; j >= 1; j--) {
        const XyzzC p = o[j];
        if (p.is_inf()) {
            r[j] = G1B::inf();
            continue;
        }
        const CF izzz = inv * CF{r[j].x};
        inv = inv * p.zzz;
        const CF izz = sqr(izzz) * sqr(p.zz);
        r[j] = G1B{(p.x * izz).v, (p.y * izzz).v};
    }
}
__global__ void __launch_bounds__(64) k_g16b_pub_partial(size_t n, size_t nsc, size_t nw, size_t nc, size_t nslices,
                                                         const G1B* table, const FrBls* wit, const FrBls* hashes,
                                                         XyzzC* part) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n * nslices) return;
    const size_t p = id / nslices, s = id - p * nslices;
    const size_t t1 = (s + 1) * kSliceB < nsc ? (s + 1) * kSliceB : nsc;
    XyzzC acc = XyzzC::inf();
    for (size_t t = s * kSliceB; t < t1; t++) {
        // scalar t of proof p: the public witness, then the commitment hashes
        FrBls x = from_mont(t < nw ? wit[p * nw + t] : hashes[p * nc + (t - nw)]);
        for (int w = 0; w < 32; w++) {  // the low byte, then the scalar moves down by 8 bits
            const uint32_t j = x.v[0] & 0xffu;
            if (j) {
                const G1C q = to_c(table[(t * 32 + (size_t)w) * 256 + j]);
                if (!q.is_inf()) xyzz_madd_inplace(acc, q);
            }
#pragma unroll
            for (int q = 0; q < 7; q++) x.v[q] = (x.v[q] >> 8) | (x.v[q + 1] << 24);
            x.v[7] >>= 8;
        }
    }
    part[id] = acc;
}

__global__ void __launch_bounds__(64) k_g1_check_endo_bls(size_t n, const G1B* p, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g1_check_endo<TwB>(p[i]);
}
__global__ void __launch_bounds__(64) k_g2_check_endo_bls(size_t n, const G2B* q, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g2_check_endo<TwB>(q[i]);
}

// ------------------------------------------------------------------ host side
// the canonical value, big-endian, 4 bytes per limb
template <class F>
static void fe_to_be(const F& mont, uint8_t* out) {
    constexpr int N = sizeof(F) / 4;
    const F c = from_mont(mont);
    for (int i = 0; i < 4 * N; i++) out[i] = (uint8_t)(c.v[N - 1 - i / 4] >> (8 * (3 - i % 4)));
}
static const uint8_t kCommitmentDstB[] = "bsb22-commitment";  // constraint/commitment.go:7

}  // namespace pairing
}  // namespace gg

using namespace gg;
using namespace gg::pairing;

struct gg_groth16_vk_bls {
    size_t n_K = 0, nb_public = 0, nc = 0;
    std::vector<uint32_t> coff, cidx;
    // the host copy: usable by _host where there is no GPU
    std::vector<G1B> K;
    std::vector<LineB> lines;  // -delta, -gamma, G, GRootSigmaNeg (kLinesB each)
    GTB e;                     // e(alpha, beta)^3
    std::mutex mu;             // one batch at a time per key: the buffers below are the key's
    bool uploaded = false;
    int device = 0;
    hipStream_t st = nullptr;
    DevBuf dK, table, dlines, de;
    DevBuf proofs, cmts, poks, wit, hashes, chal, part, ksum, folded, status;
    ~gg_groth16_vk_bls() {
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

// the commitment hashes and the folding challenge (verify.go:80-100), host pointers
void commitment_hashes(const gg_groth16_vk_bls* vk, size_t n, const G1B* C, const FrBls* W,
                       std::vector<FrBls>& hashes, std::vector<uint32_t>& chal) {
    const size_t nc = vk->nc, nw = vk->nb_public - 1;
    hashes.assign(n * nc, FrBls::zero());
    chal.assign(nc > 1 ? n * 8 : 0, 0);
    if (!nc) return;
    std::vector<uint8_t> msg, ser(1 + 32 * nc);
    ser[0] = 'r';
    for (size_t i = 0; i < n; i++) {
        for (size_t j = 0; j < nc; j++) {
            const uint32_t t0 = vk->coff[j], t1 = vk->coff[j + 1];
            msg.assign(96 + 32 * (size_t)(t1 - t0), 0);
            const G1B& c = C[i * nc + j];
            if (c.is_inf()) {
                msg[0] = 0x40;  // RawEncoding's infinity flag
            } else {
                fe_to_be(c.x, msg.data());
                fe_to_be(c.y, msg.data() + 48);
            }
            for (uint32_t t = t0; t < t1; t++) {
                const size_t idx = vk->cidx[t] - 1;  // into the witness extended by the earlier hashes
                fe_to_be(idx < nw ? W[i * nw + idx] : hashes[i * nc + (idx - nw)], msg.data() + 96 + 32 * (t - t0));
            }
            const FrBls h = hash_to_field_bls(msg.data(), msg.size(), kCommitmentDstB, sizeof(kCommitmentDstB) - 1);
            hashes[i * nc + j] = h;
            fe_to_be(h, ser.data() + 1 + 32 * j);
        }
        if (nc > 1) {  // pedersen getChallenge: sha256("r" | hashes) mod r
            uint8_t d[32];
            Sha256::hash(ser.data(), ser.size(), d);
            const FrBls r = from_mont(frb_from_be(d, 32));
            memcpy(&chal[8 * i], r.v, 32);
        }
    }
}

void check_batch_args(gg_groth16_vk_bls* vk, size_t n, const void* proofs, const void* commitments, const void* poks,
                      const void* public_witness, const uint8_t* status_out) {
    GG_CHECK(vk, GG_ERR_INVALID_ARG, "null argument: vk");
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(n <= ((size_t)1 << 24), GG_ERR_INVALID_ARG, "n exceeds 2^24 proofs per call");
    GG_CHECK(proofs, GG_ERR_INVALID_ARG, "null argument: proofs");
    GG_CHECK(status_out, GG_ERR_INVALID_ARG, "null argument: status_out");
    GG_CHECK(commitments || !vk->nc, GG_ERR_INVALID_ARG, "null argument: commitments (the key has commitments)");
    GG_CHECK(poks || !vk->nc, GG_ERR_INVALID_ARG, "null argument: poks (the key has commitments)");
    GG_CHECK(public_witness || vk->nb_public == 1, GG_ERR_INVALID_ARG, "null argument: public_witness");
}

// host copy of `bytes` at p (p itself when it is host memory)
const uint8_t* to_host(const void* p, size_t bytes, std::vector<uint8_t>& buf) {
    if (!bytes || !is_device_ptr(p)) return (const uint8_t*)p;
    buf.resize(bytes);
    GG_HIP(hipMemcpy(buf.data(), p, bytes, hipMemcpyDeviceToHost));
    return buf.data();
}

// the first device batch of a key: the key's arrays and the window table of K[1:]
void upload_key(gg_groth16_vk_bls* vk) {
    GG_HIP(hipGetDevice(&vk->device));
    if (!vk->st) GG_HIP(hipStreamCreateWithFlags(&vk->st, hipStreamNonBlocking));
    hipStream_t st = vk->st;
    vk->dlines.alloc(vk->lines.size() * sizeof(LineB));
    GG_HIP(hipMemcpyAsync(vk->dlines.p, vk->lines.data(), vk->dlines.bytes, hipMemcpyHostToDevice, st));
    vk->dK.alloc(vk->n_K * sizeof(G1B));
    GG_HIP(hipMemcpyAsync(vk->dK.p, vk->K.data(), vk->dK.bytes, hipMemcpyHostToDevice, st));
    vk->de.alloc(sizeof(GTB));
    GG_HIP(hipMemcpyAsync(vk->de.p, &vk->e, sizeof(GTB), hipMemcpyHostToDevice, st));
    const size_t nsc = vk->n_K - 1;
    DevBuf cur;
    if (nsc) {
        const size_t ne = nsc * 32 * 256;
        cur.alloc(ne * sizeof(XyzzC));
        vk->table.alloc(ne * sizeof(G1B));
        hipLaunchKernelGGL(k_g16b_table, dim3(grid_for(nsc * 32, 64)), dim3(64), 0, st, vk->dK.as<G1B>(), nsc,
                           cur.as<XyzzC>(), vk->table.as<G1B>());
        GG_HIP(hipGetLastError());
    }
    GG_WAIT_STREAM(st);
    vk->uploaded = true;
}

}  // namespace

extern "C" int gg_groth16_vk_create_bls12_381(const void* alpha1, const void* beta2, const void* gamma2,
                                              const void* delta2, const void* K, size_t n_K, size_t nb_public,
                                              const void* ped_g, const void* ped_g_root_sigma_neg,
                                              const uint32_t* committed_off, const uint32_t* committed_idx,
                                              int n_commitments, gg_groth16_vk_bls_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    GG_CHECK(alpha1, GG_ERR_INVALID_ARG, "null argument: alpha1");
    GG_CHECK(beta2, GG_ERR_INVALID_ARG, "null argument: beta2");
    GG_CHECK(gamma2, GG_ERR_INVALID_ARG, "null argument: gamma2");
    GG_CHECK(delta2, GG_ERR_INVALID_ARG, "null argument: delta2");
    GG_CHECK(K, GG_ERR_INVALID_ARG, "null argument: K");
    GG_CHECK(nb_public >= 1, GG_ERR_INVALID_ARG, "nb_public must be >= 1 (it counts the ONE wire)");
    GG_CHECK(n_commitments >= 0, GG_ERR_INVALID_ARG, "n_commitments must be >= 0");
    const size_t nc = (size_t)n_commitments;
    GG_CHECK(n_K == nb_public + nc, GG_ERR_INVALID_ARG,
             "n_K = " + std::to_string(n_K) + " but nb_public + n_commitments = " + std::to_string(nb_public + nc));
    GG_CHECK(n_K <= GG_VERIFY_MAX_K, GG_ERR_INVALID_ARG,
             "n_K = " + std::to_string(n_K) + " exceeds GG_VERIFY_MAX_K = " + std::to_string(GG_VERIFY_MAX_K));
    std::unique_ptr<gg_groth16_vk_bls> vk(new gg_groth16_vk_bls);
    if (nc) {
        GG_CHECK(ped_g, GG_ERR_INVALID_ARG, "null argument: ped_g");
        GG_CHECK(ped_g_root_sigma_neg, GG_ERR_INVALID_ARG, "null argument: ped_g_root_sigma_neg");
        GG_CHECK(committed_off, GG_ERR_INVALID_ARG, "null argument: committed_off");
        GG_CHECK(committed_off[0] == 0, GG_ERR_INVALID_ARG, "committed_off[0] must be 0");
        for (size_t j = 0; j < nc; j++)
            GG_CHECK(committed_off[j] <= committed_off[j + 1], GG_ERR_INVALID_ARG, "committed_off must not decrease");
        GG_CHECK(committed_idx || !committed_off[nc], GG_ERR_INVALID_ARG, "null argument: committed_idx");
        for (size_t j = 0; j < nc; j++)
            for (uint32_t t = committed_off[j]; t < committed_off[j + 1]; t++)
                GG_CHECK(committed_idx[t] >= 1 && committed_idx[t] < nb_public + j, GG_ERR_INVALID_ARG,
                         "committed index " + std::to_string(committed_idx[t]) + " of commitment " + std::to_string(j) +
                             " out of range [1, " + std::to_string(nb_public + j) + ")");
        vk->coff.assign(committed_off, committed_off + nc + 1);
        vk->cidx.assign(committed_idx, committed_idx + committed_off[nc]);
    }
    G2B q[4];
    memcpy(&q[0], delta2, sizeof(G2B));
    memcpy(&q[1], gamma2, sizeof(G2B));
    GG_CHECK(!q[0].is_inf(), GG_ERR_INVALID_ARG, "delta2 is the point at infinity");
    GG_CHECK(!q[1].is_inf(), GG_ERR_INVALID_ARG, "gamma2 is the point at infinity");
    q[0] = neg(q[0]);
    q[1] = neg(q[1]);
    int nq = 2;
    if (nc) {
        memcpy(&q[2], ped_g, sizeof(G2B));
        memcpy(&q[3], ped_g_root_sigma_neg, sizeof(G2B));
        GG_CHECK(!q[2].is_inf(), GG_ERR_INVALID_ARG, "ped_g is the point at infinity");
        GG_CHECK(!q[3].is_inf(), GG_ERR_INVALID_ARG, "ped_g_root_sigma_neg is the point at infinity");
        nq = 4;
    }
    vk->n_K = n_K;
    vk->nb_public = nb_public;
    vk->nc = nc;
    vk->K.resize(n_K);
    memcpy(vk->K.data(), K, n_K * sizeof(G1B));
    // the fixed operands' lines and e(alpha, beta)^3, by the templates the kernels run
    vk->lines.resize((size_t)4 * kLinesB);
    for (int t = 0; t < nq; t++) line_table<TwB>(q[t], vk->lines.data() + (size_t)t * kLinesB);
    G1B a;
    G2B b;
    memcpy(&a, alpha1, sizeof(G1B));
    memcpy(&b, beta2, sizeof(G2B));
    vk->e = pairing_product<TwB>(1, &a, &b);
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_groth16_vk_destroy_bls12_381(gg_groth16_vk_bls_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

extern "C" int gg_groth16_verify_batch_bls12_381_host(gg_groth16_vk_bls_t vk, size_t n, const void* proofs,
                                                      const void* commitments, const void* poks,
                                                      const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    check_batch_args(vk, n, proofs, commitments, poks, public_witness, status_out);
    const size_t nc = vk->nc, nw = vk->nb_public - 1, nsc = vk->n_K - 1;
    const FrBls* W = (const FrBls*)public_witness;
    std::vector<FrBls> hashes;
    std::vector<uint32_t> chal;
    commitment_hashes(vk, n, (const G1B*)commitments, W, hashes, chal);
    // the public-input sum by plain scalar multiplication: one partial sum per proof
    const size_t nslices = nsc ? 1 : 0;
    std::vector<XyzzC> part(n * nslices);
    for (size_t i = 0; i < n && nsc; i++) {
        JacC acc = JacC::inf();
        for (size_t t = 0; t < nsc; t++) {
            const FrBls x = from_mont(t < nw ? W[i * nw + t] : hashes[i * nc + (t - nw)]);
            acc = jac_add(acc, g1_mul_words_c(JacC::from_affine(to_c(vk->K[t + 1])), x.v));
        }
        part[i] = jac_to_xyzz(acc);
    }
    std::vector<G1B> ksum(n), folded(nc ? n : 0);
    const LineB* L = vk->lines.data();
    const G16Args a{n, nc, nslices, (const ProofB*)proofs, (const G1B*)commitments, (const G1B*)poks, vk->K.data(),
                    part.data(), chal.data(), ksum.data(), folded.data(), status_out,
                    L, L + kLinesB, L + 2 * kLinesB, L + 3 * kLinesB, &vk->e};
    for (size_t i = 0; i < n; i++) {
        g16_prep_one(a, i);
        g16_pair_one(a, i);
    }
    GG_CAPI_END
}

extern "C" int gg_groth16_verify_batch_bls12_381(gg_groth16_vk_bls_t vk, size_t n, const void* proofs,
                                                 const void* commitments, const void* poks,
                                                 const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    check_batch_args(vk, n, proofs, commitments, poks, public_witness, status_out);
    const size_t nc = vk->nc, nw = vk->nb_public - 1, nsc = vk->n_K - 1;
    std::lock_guard<std::mutex> lock(vk->mu);
    if (!vk->uploaded) upload_key(vk);
    GG_HIP(hipSetDevice(vk->device));
    hipStream_t st = vk->st;
    std::vector<FrBls> hashes;
    std::vector<uint32_t> chal;
    {
        std::vector<uint8_t> hb_c, hb_w;
        const G1B* C = nc ? (const G1B*)to_host(commitments, n * nc * sizeof(G1B), hb_c) : nullptr;
        const FrBls* W = nc ? (const FrBls*)to_host(public_witness, n * nw * sizeof(FrBls), hb_w) : nullptr;
        commitment_hashes(vk, n, C, W, hashes, chal);
    }
    const size_t nslices = (nsc + kSliceB - 1) / kSliceB;
    G16Args a{};
    a.n = n;
    a.nc = nc;
    a.nslices = nslices;
    a.proofs = (const ProofB*)to_device(proofs, n * sizeof(ProofB), vk->proofs, st);
    a.cmts = (const G1B*)to_device(commitments, n * nc * sizeof(G1B), vk->cmts, st);
    a.poks = (const G1B*)to_device(poks, nc ? n * sizeof(G1B) : 0, vk->poks, st);
    const FrBls* dw = (const FrBls*)to_device(public_witness, n * nw * sizeof(FrBls), vk->wit, st);
    if (nc) {
        vk->hashes.reserve(hashes.size() * sizeof(FrBls));
        GG_HIP(hipMemcpyAsync(vk->hashes.p, hashes.data(), hashes.size() * sizeof(FrBls), hipMemcpyHostToDevice, st));
    }
    if (!chal.empty()) {
        vk->chal.reserve(chal.size() * 4);
        GG_HIP(hipMemcpyAsync(vk->chal.p, chal.data(), chal.size() * 4, hipMemcpyHostToDevice, st));
    }
    vk->ksum.reserve(n * sizeof(G1B));
    if (nc) vk->folded.reserve(n * sizeof(G1B));
    OutBuf so;
    if (is_device_ptr(status_out)) {
        so.dev = status_out;
    } else {
        vk->status.reserve(n);
        so.host = status_out;
        so.dev = vk->status.p;
    }
    so.bytes = n;
    if (nslices) {
        vk->part.reserve(n * nslices * sizeof(XyzzC));
        hipLaunchKernelGGL(k_g16b_pub_partial, dim3(grid_for(n * nslices, 64)), dim3(64), 0, st, n, nsc, nw, nc,
                           nslices, vk->table.as<G1B>(), dw, vk->hashes.as<FrBls>(), vk->part.as<XyzzC>());
        GG_HIP(hipGetLastError());
    }
    a.K = vk->dK.as<G1B>();
    a.part = vk->part.as<XyzzC>();
    a.chal = vk->chal.as<uint32_t>();
    a.ksum = vk->ksum.as<G1B>();
    a.folded = vk->folded.as<G1B>();
    a.status = (uint8_t*)so.dev;
    const LineB* L = vk->dlines.as<LineB>();
    a.delta_neg = L;
    a.gamma_neg = L + kLinesB;
    a.ped_g = L + 2 * kLinesB;
    a.ped_gs = L + 3 * kLinesB;
    a.e = vk->de.as<GTB>();
    hipLaunchKernelGGL(k_g16b_prep, dim3(grid_for(n, 64)), dim3(64), 0, st, a);
    GG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_g16b_pair, dim3(grid_for(n, 64)), dim3(64), 0, st, a);
    GG_HIP(hipGetLastError());
    so.finish(st);
    GG_CAPI_END
}

extern "C" int gg_hash_to_field_bls12_381(const void* msg, size_t len, const void* dst, size_t dst_len, void* out32) {
    GG_CAPI_BEGIN
    GG_CHECK(msg || !len, GG_ERR_INVALID_ARG, "null argument: msg");
    GG_CHECK(dst || !dst_len, GG_ERR_INVALID_ARG, "null argument: dst");
    GG_CHECK(out32, GG_ERR_INVALID_ARG, "null argument: out32");
    GG_CHECK(dst_len <= 255, GG_ERR_INVALID_ARG, "dst_len must be <= 255 (expand_message_xmd)");
    const FrBls h = hash_to_field_bls((const uint8_t*)msg, len, (const uint8_t*)dst, dst_len);
    memcpy(out32, &h, 32);
    GG_CAPI_END
}
extern "C" int gg_g1_check_endo_bls12_381(size_t n, const void* g1, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g1, "g1", flags_out);
    run_check<G1B>(n, g1, flags_out, k_g1_check_endo_bls, 64);
    GG_CAPI_END
}
extern "C" int gg_g2_check_endo_bls12_381(size_t n, const void* g2, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g2, "g2", flags_out);
    run_check<G2B>(n, g2, flags_out, k_g2_check_endo_bls, 64);
    GG_CAPI_END
}
