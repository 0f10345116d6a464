// Groth16 Verify for batches of proofs under one verifying key
// (backend/groth16/<curve>/verify.go:42-140), BSB22 commitments included, for any
// curve described by a traits struct C: groth16_verify.hip instantiates it for
// BN254, groth16_verify_bls.hip for BLS12-381.
//
// Every step is a per-lane GG_HD function; a kernel runs it over a grid and the
// host path over a loop, on the same arrays.  One lane per proof, 64-lane
// blocks; the Fp12 / Fp6 routines of pairing.cuh are real calls and their
// operands live in the lane's stack frame (scratch).
//
//   table_lane       lane (t, w): T[t][w][j] = j 2^(8w) K[t + 1], j < 256, built in
//                    XYZZ and normalised to affine with one inversion per lane
//   pub_partial_one  lane (proof, slice of kSlice public inputs): 32 mixed
//                    additions per scalar from the table, no doubling; exact for
//                    0 and r - 1, and for a K[t + 1] at infinity
//   prep_one         per proof: the point checks, kSum, the folded commitment
//   pair_one         per proof: the Pedersen check, then the 3-pair Miller loop
//                    with the key's line tables for -delta and -gamma, the final
//                    exponentiation and the comparison with e(alpha, beta)^m
//
// Per batch: the commitment hashes and the folding challenge on the host; then
// pub_partial_one, prep_one and pair_one on the device.  The host path has no
// table: its public-input sum is a plain scalar multiplication per input.
// create_key validates everything and precomputes on the host, with no device
// call; upload_key copies the key to the current device and builds the table.
// DESIGN.md §4 "Groth16 Verify".
//
// The traits struct C gives
//   Tw            the pairing tower (pairing.cuh); Tw::F is the stored coordinate
//   Fr            the scalar field
//   PC            the coordinate type of the point loops: Tw::F, or Called<Tw::F>
//                 (the same bytes) where an inlined loop body would outgrow a
//                 short branch
//   inv(PC)       the inversion of the affine results
//   g1_flag, g2_flag   0 good, 1 off the curve, 2 outside the r-torsion
//   kPubBlock     the block size of the pub_partial_one kernel
// and Kernels<C> (specialised beside the kernels) names the __global__ wrappers.
#pragma once
#include "common.h"
#include "pairing.cuh"
#include "pairing_host.h"
#include "pairing_run.h"
#include "sha256.h"
#include "transcript.h"
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace gg {
namespace groth16v {

using namespace gg::pairing;
constexpr size_t kSlice = 8;  // public inputs per lane of pub_partial_one
static const uint8_t kCommitmentDst[] = "bsb22-commitment";  // constraint/commitment.go:7

template <class F>
GG_HD const F& raw(const F& a) {
    return a;
}
template <class F>
GG_HD const F& raw(const Called<F>& a) {
    return a.v;
}

template <class C>
struct Kernels;

template <class C>
struct Verifier {
    using Tw = typename C::Tw;
    using Fr = typename C::Fr;
    using PC = typename C::PC;
    using F = typename Tw::F;
    using G1A = Affine<F>;  // as stored
    using G2A = Affine<typename Tw::F2>;
    using G1P = Affine<PC>;  // as the point loops read it
    using XZ = Xyzz<PC>;
    using JacP = Jac<PC>;
    using GT = Fp12<Tw>;
    using LineT = Line<Tw>;
    static constexpr int kLines = line_count<Tw>();
    static_assert(sizeof(PC) == sizeof(F) && sizeof(Fr) == 32, "one point layout, 32-byte scalars");

    struct Proof {
        G1A ar;
        G2A bs;
        G1A krs;
    };

    static GG_HD G1P to_c(const G1A& a) { return G1P{PC{a.x}, PC{a.y}}; }
    static GG_HD G1A xyzz_to_affine(const XZ& p) {
        if (p.is_inf()) return G1A::inf();
        const PC i3 = C::inv(p.zzz);
        return G1A{raw(p.x * sqr(p.zz * i3)), raw(p.y * i3)};
    }
    static GG_HD G1A jac_to_affine(const JacP& p) {
        if (p.is_inf()) return G1A::inf();
        const PC zi = C::inv(p.z);
        const PC zi2 = sqr(zi);
        return G1A{raw(p.x * zi2), raw(p.y * zi2 * zi)};
    }
    // k a for a canonical scalar of 8 words
    static GG_HDN JacP g1_mul_words(const JacP& a, const uint32_t* k) {
        JacP acc = JacP::inf();
        for (int wd = 7; wd >= 0; wd--) {
            const uint32_t word = k[wd];
            for (int b = 31; b >= 0; b--) {
                acc = jac_dbl(acc);
                if ((word >> b) & 1) acc = jac_add(acc, a);
            }
        }
        return acc;
    }

    // ------------------------------------------------------------ per-lane steps
    struct TableArgs {
        const G1A* K;
        size_t nsc;
        XZ* cur;   // nsc x 32 x 256: the lane's multiples before the inversion
        G1A* out;  // the table; the prefix products wait in the x coordinate of their slot
    };
    static GG_HD void table_lane(const TableArgs& a, size_t id) {
        const size_t t = id >> 5;
        const int w = (int)(id & 31);
        XZ b = XZ::from_affine(to_c(a.K[t + 1]));
        for (int s = 0; s < 8 * w; s++) b = xyzz_dbl(b);
        XZ* o = a.cur + id * 256;
        G1A* r = a.out + id * 256;
        XZ acc = b;
        PC prod = PC::one();
        r[0] = G1A::inf();
        for (int j = 1; j < 256; j++) {
            o[j] = acc;
            r[j].x = raw(prod);
            if (!acc.is_inf()) prod = prod * acc.zzz;
            acc = xyzz_add(acc, b);
        }
        PC inv = C::inv(prod);
        for (int j = 255; j >= 1; j--) {
            const XZ p = o[j];
            if (p.is_inf()) {
                r[j] = G1A::inf();
                continue;
            }
            const PC izzz = inv * PC{r[j].x};
            inv = inv * p.zzz;
            const PC izz = sqr(izzz) * sqr(p.zz);
            r[j] = G1A{raw(p.x * izz), raw(p.y * izzz)};
        }
    }

    struct PubArgs {
        size_t n, nsc, nw, nc, nslices;
        const G1A* table;
        const Fr *wit, *hashes;  // scalar t of a proof: the public witness, then the commitment hashes
        XZ* part;
    };
    static GG_HD void pub_partial_one(const PubArgs& a, size_t id) {
        const size_t p = id / a.nslices, s = id - p * a.nslices;
        const size_t t1 = (s + 1) * kSlice < a.nsc ? (s + 1) * kSlice : a.nsc;
        XZ acc = XZ::inf();
        for (size_t t = s * kSlice; t < t1; t++) {
            Fr x = from_mont(t < a.nw ? a.wit[p * a.nw + t] : a.hashes[p * a.nc + (t - a.nw)]);
            for (int w = 0; w < 32; w++) {  // the low byte, then the scalar moves down by 8 bits
                const uint32_t j = x.v[0] & 0xffu;
                if (j) {  // a K[t + 1] at infinity (an input no constraint uses) has an all-infinity row
                    const G1P q = to_c(a.table[(t * 32 + (size_t)w) * 256 + j]);
                    if (!q.is_inf()) xyzz_madd_inplace(acc, q);
                }
#pragma unroll
                for (int q = 0; q < 7; q++) x.v[q] = (x.v[q] >> 8) | (x.v[q + 1] << 24);
                x.v[7] >>= 8;
            }
        }
        a.part[id] = acc;
    }

    // what prep_one and pair_one read and write: the batch, the key, the work arrays
    struct Args {
        size_t n, nc, nslices;
        const Proof* proofs;
        const G1A *cmts, *poks, *K;
        const XZ* part;        // n x nslices partial public-input sums
        const uint32_t* chal;  // n x 8 words: the folding challenge, canonical (nc > 1)
        G1A *ksum, *folded;
        uint8_t* status;
        const LineT *delta_neg, *gamma_neg, *ped_g, *ped_gs;
        const GT* e;
    };
    // proof.isValid (verify.go:61), kSum (110-119) and the folded commitment
    static GG_HD void prep_one(const Args& a, size_t i) {
        const Proof& pr = a.proofs[i];
        const size_t nc = a.nc;
        bool bad = C::g1_flag(pr.ar) != 0;
        if (!bad) bad = C::g1_flag(pr.krs) != 0;
        for (size_t j = 0; j < nc && !bad; j++) bad = C::g1_flag(a.cmts[i * nc + j]) != 0;
        if (nc && !bad) bad = C::g1_flag(a.poks[i]) != 0;
        if (!bad) bad = C::g2_flag(pr.bs) != 0;
        if (bad) {
            a.status[i] = GG_VERIFY_SUBGROUP;
            return;
        }
        XZ acc = XZ::from_affine(to_c(a.K[0]));
        for (size_t s = 0; s < a.nslices; s++) xyzz_add_inplace(acc, a.part[i * a.nslices + s]);
        for (size_t j = 0; j < nc; j++) {
            const G1P c = to_c(a.cmts[i * nc + j]);
            if (!c.is_inf()) xyzz_madd_inplace(acc, c);
        }
        a.ksum[i] = xyzz_to_affine(acc);
        if (nc) {  // sum_j r^j C_j by Horner (pedersen.FoldCommitments; one commitment: itself)
            JacP f = JacP::from_affine(to_c(a.cmts[i * nc + nc - 1]));
            for (size_t j = nc - 1; j-- > 0;)
                f = jac_add(g1_mul_words(f, a.chal + 8 * i), JacP::from_affine(to_c(a.cmts[i * nc + j])));
            a.folded[i] = jac_to_affine(f);
        }
        a.status[i] = GG_VERIFY_OK;
    }
    // the Pedersen check (verify.go:105), then the pairing equation (124-135)
    static GG_HD void pair_one(const Args& a, size_t i) {
        if (a.status[i] != GG_VERIFY_OK) return;
        G1A p[3];
        G2Src<Tw> s[3];
        if (a.nc) {  // e(folded, G) e(pok, GRootSigmaNeg) == 1
            p[0] = a.folded[i];
            p[1] = a.poks[i];
            s[0].tab = a.ped_g;
            s[0].skip = p[0].is_inf();
            s[1].tab = a.ped_gs;
            s[1].skip = p[1].is_inf();
            GT f = GT::one();
            miller_loop<Tw, 2>(f, p, s);
            if (!final_exp(f).is_one()) {
                a.status[i] = GG_VERIFY_PEDERSEN;
                return;
            }
        }
        const Proof& pr = a.proofs[i];
        p[0] = pr.krs;
        p[1] = pr.ar;
        p[2] = a.ksum[i];
        s[0].tab = a.delta_neg;
        s[0].pos = 0;
        s[0].skip = p[0].is_inf();
        src_init<Tw>(s[1], pr.bs, nullptr, p[1].is_inf());
        s[2].tab = a.gamma_neg;
        s[2].pos = 0;
        s[2].skip = p[2].is_inf();
        GT f = GT::one();
        miller_loop<Tw, 3>(f, p, s);
        a.status[i] = final_exp(f) == *a.e ? GG_VERIFY_OK : GG_VERIFY_PAIRING;
    }

    // ------------------------------------------------------------ host side
    struct Key {
        size_t n_K = 0, nb_public = 0, nc = 0;
        std::vector<uint32_t> coff, cidx;
        // the host copy: all the host path needs
        std::vector<G1A> K;
        std::vector<LineT> lines;  // -delta, -gamma, G, GRootSigmaNeg (kLines each)
        GT e;                      // e(alpha, beta)^m
        std::mutex mu;             // one device batch at a time per key: the buffers below are the key's
        bool uploaded = false;
        int device = 0;
        hipStream_t st = nullptr;
        DevBuf dK, table, dlines, de;
        DevBuf proofs, cmts, poks, wit, hashes, chal, part, ksum, folded, status;
        ~Key() {
            if (st) (void)hipStreamDestroy(st);
        }
    };

    // validates everything and fills *vk; no device call
    static void create_key(Key* vk, const void* alpha1, const void* beta2, const void* gamma2, const void* delta2,
                           const void* K, size_t n_K, size_t nb_public, const void* ped_g,
                           const void* ped_g_root_sigma_neg, const uint32_t* committed_off,
                           const uint32_t* committed_idx, int n_commitments) {
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
        if (nc) {
            GG_CHECK(ped_g, GG_ERR_INVALID_ARG, "null argument: ped_g");
            GG_CHECK(ped_g_root_sigma_neg, GG_ERR_INVALID_ARG, "null argument: ped_g_root_sigma_neg");
            GG_CHECK(committed_off, GG_ERR_INVALID_ARG, "null argument: committed_off");
            GG_CHECK(committed_off[0] == 0, GG_ERR_INVALID_ARG, "committed_off[0] must be 0");
            for (size_t j = 0; j < nc; j++)
                GG_CHECK(committed_off[j] <= committed_off[j + 1], GG_ERR_INVALID_ARG,
                         "committed_off must not decrease");
            GG_CHECK(committed_idx || !committed_off[nc], GG_ERR_INVALID_ARG, "null argument: committed_idx");
            for (size_t j = 0; j < nc; j++)
                for (uint32_t t = committed_off[j]; t < committed_off[j + 1]; t++)
                    GG_CHECK(committed_idx[t] >= 1 && committed_idx[t] < nb_public + j, GG_ERR_INVALID_ARG,
                             "committed index " + std::to_string(committed_idx[t]) + " of commitment " +
                                 std::to_string(j) + " out of range [1, " + std::to_string(nb_public + j) + ")");
            vk->coff.assign(committed_off, committed_off + nc + 1);
            vk->cidx.assign(committed_idx, committed_idx + committed_off[nc]);
        }
        G2A q[4];
        memcpy(&q[0], delta2, sizeof(G2A));
        memcpy(&q[1], gamma2, sizeof(G2A));
        GG_CHECK(!q[0].is_inf(), GG_ERR_INVALID_ARG, "delta2 is the point at infinity");
        GG_CHECK(!q[1].is_inf(), GG_ERR_INVALID_ARG, "gamma2 is the point at infinity");
        q[0] = neg(q[0]);
        q[1] = neg(q[1]);
        int nq = 2;
        if (nc) {
            memcpy(&q[2], ped_g, sizeof(G2A));
            memcpy(&q[3], ped_g_root_sigma_neg, sizeof(G2A));
            GG_CHECK(!q[2].is_inf(), GG_ERR_INVALID_ARG, "ped_g is the point at infinity");
            GG_CHECK(!q[3].is_inf(), GG_ERR_INVALID_ARG, "ped_g_root_sigma_neg is the point at infinity");
            nq = 4;
        }
        vk->n_K = n_K;
        vk->nb_public = nb_public;
        vk->nc = nc;
        vk->K.resize(n_K);
        memcpy(vk->K.data(), K, n_K * sizeof(G1A));
        // the fixed operands' lines and e(alpha, beta)^m, by the templates the kernels run
        vk->lines.resize((size_t)4 * kLines);
        for (int t = 0; t < nq; t++) line_table<Tw>(q[t], vk->lines.data() + (size_t)t * kLines);
        G1A a;
        G2A b;
        memcpy(&a, alpha1, sizeof(G1A));
        memcpy(&b, beta2, sizeof(G2A));
        vk->e = pairing_product<Tw>(1, &a, &b);
    }

    // binds the key to the current device: its arrays and the window table of K[1:]
    static void upload_key(Key* vk) {
        GG_HIP(hipGetDevice(&vk->device));
        if (!vk->st) GG_HIP(hipStreamCreateWithFlags(&vk->st, hipStreamNonBlocking));
        hipStream_t st = vk->st;
        upload(vk->dlines, vk->lines.data(), vk->lines.size() * sizeof(LineT), st);
        upload(vk->dK, vk->K.data(), vk->n_K * sizeof(G1A), st);
        upload(vk->de, &vk->e, sizeof(GT), st);
        const size_t nsc = vk->n_K - 1, ne = nsc * 32 * 256;
        DevBuf cur(ne * sizeof(XZ));
        vk->table.alloc(ne * sizeof(G1A));
        const TableArgs ta{vk->dK.template as<G1A>(), nsc, cur.template as<XZ>(), vk->table.template as<G1A>()};
        run(true, st, Kernels<C>::table, table_lane, ta, nsc * 32, 64);
        GG_WAIT_STREAM(st);
        vk->uploaded = true;
    }

    template <class FF>
    static void be(const FF& mont, uint8_t* out) {
        fs::be_bytes<sizeof(FF) / 4>(from_mont(mont).v, out);
    }
    // the commitment hashes and the folding challenge (verify.go:80-100), host pointers
    static void commitment_hashes(const Key* vk, size_t n, const G1A* cmts, const Fr* W, std::vector<Fr>& hashes,
                                  std::vector<uint32_t>& chal) {
        const size_t nc = vk->nc, nw = vk->nb_public - 1, pt = sizeof(G1A);
        hashes.assign(n * nc, Fr::zero());
        chal.assign(nc > 1 ? n * 8 : 0, 0);
        if (!nc) return;
        std::vector<uint8_t> msg, ser(1 + 32 * nc);
        ser[0] = 'r';
        for (size_t i = 0; i < n; i++) {
            for (size_t j = 0; j < nc; j++) {
                const uint32_t t0 = vk->coff[j], t1 = vk->coff[j + 1];
                msg.assign(pt + 32 * (size_t)(t1 - t0), 0);  // Marshal(C_j), then the committed values
                const G1A& c = cmts[i * nc + j];
                if (c.is_inf()) {
                    msg[0] = 0x40;  // RawEncoding's infinity flag
                } else {
                    be(c.x, msg.data());
                    be(c.y, msg.data() + pt / 2);
                }
                for (uint32_t t = t0; t < t1; t++) {
                    const size_t idx = vk->cidx[t] - 1;  // into the witness extended by the earlier hashes
                    be(idx < nw ? W[i * nw + idx] : hashes[i * nc + (idx - nw)], msg.data() + pt + 32 * (t - t0));
                }
                const Fr h = hash_to_field<Fr>(msg.data(), msg.size(), kCommitmentDst, sizeof(kCommitmentDst) - 1);
                hashes[i * nc + j] = h;
                be(h, ser.data() + 1 + 32 * j);
            }
            if (nc > 1) {  // pedersen getChallenge: sha256("r" | hashes) mod r
                uint8_t d[32];
                Sha256::hash(ser.data(), ser.size(), d);
                const Fr r = from_mont(fr_from_be<Fr>(d, 32));
                memcpy(&chal[8 * i], r.v, 32);
            }
        }
    }

    static void check_batch_args(const Key* vk, size_t n, const void* proofs, const void* commitments,
                                 const void* poks, const void* public_witness, const uint8_t* status_out) {
        GG_CHECK(vk, GG_ERR_INVALID_ARG, "null argument: vk");
        GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
        GG_CHECK(n <= ((size_t)1 << 24), GG_ERR_INVALID_ARG, "n exceeds 2^24 proofs per call");
        GG_CHECK(proofs, GG_ERR_INVALID_ARG, "null argument: proofs");
        GG_CHECK(status_out, GG_ERR_INVALID_ARG, "null argument: status_out");
        GG_CHECK(commitments || !vk->nc, GG_ERR_INVALID_ARG, "null argument: commitments (the key has commitments)");
        GG_CHECK(poks || !vk->nc, GG_ERR_INVALID_ARG, "null argument: poks (the key has commitments)");
        GG_CHECK(public_witness || vk->nb_public == 1, GG_ERR_INVALID_ARG, "null argument: public_witness");
    }

    // dev: the arrays may be host or device memory; else host memory, and no device call
    static void verify_batch(Key* vk, bool dev, size_t n, const void* proofs, const void* commitments,
                             const void* poks, const void* public_witness, uint8_t* status_out) {
        check_batch_args(vk, n, proofs, commitments, poks, public_witness, status_out);
        const size_t nc = vk->nc, nw = vk->nb_public - 1, nsc = vk->n_K - 1;
        std::unique_lock<std::mutex> lock(vk->mu, std::defer_lock);
        hipStream_t st = nullptr;
        if (dev) {
            lock.lock();
            if (!vk->uploaded) upload_key(vk);
            GG_HIP(hipSetDevice(vk->device));
            st = vk->st;
        }
        const G1A* cm = (const G1A*)commitments;
        const Fr* W = (const Fr*)public_witness;
        std::vector<uint8_t> hb_c, hb_w;
        if (dev && nc) {
            cm = (const G1A*)to_host(commitments, n * nc * sizeof(G1A), hb_c);
            W = (const Fr*)to_host(public_witness, n * nw * sizeof(Fr), hb_w);
        }
        std::vector<Fr> hashes;
        std::vector<uint32_t> chal;
        commitment_hashes(vk, n, cm, W, hashes, chal);

        Args a{};
        a.n = n;
        a.nc = nc;
        const LineT* L = vk->lines.data();
        std::vector<XZ> part;
        std::vector<G1A> ksum, folded;
        OutBuf so;
        if (dev) {
            a.nslices = (nsc + kSlice - 1) / kSlice;
            a.proofs = (const Proof*)to_device(proofs, n * sizeof(Proof), vk->proofs, st);
            a.cmts = (const G1A*)to_device(commitments, n * nc * sizeof(G1A), vk->cmts, st);
            a.poks = (const G1A*)to_device(poks, nc ? n * sizeof(G1A) : 0, vk->poks, st);
            const Fr* dw = (const Fr*)to_device(public_witness, n * nw * sizeof(Fr), vk->wit, st);
            a.chal = (const uint32_t*)to_device(chal.data(), chal.size() * 4, vk->chal, st);
            const Fr* dh = (const Fr*)to_device(hashes.data(), hashes.size() * sizeof(Fr), vk->hashes, st);
            vk->part.reserve(n * a.nslices * sizeof(XZ));
            vk->ksum.reserve(n * sizeof(G1A));
            if (nc) vk->folded.reserve(n * sizeof(G1A));
            so.init(status_out, n, vk->status);
            a.K = vk->dK.template as<G1A>();
            a.part = vk->part.template as<XZ>();
            a.ksum = vk->ksum.template as<G1A>();
            a.folded = vk->folded.template as<G1A>();
            a.status = (uint8_t*)so.dev;
            a.e = vk->de.template as<GT>();
            L = vk->dlines.template as<LineT>();
            const PubArgs pa{n, nsc, nw, nc, a.nslices, vk->table.template as<G1A>(), dw, dh, vk->part.template as<XZ>()};
            run(true, st, Kernels<C>::pub, pub_partial_one, pa, n * a.nslices, C::kPubBlock);
        } else {  // the public-input sum by plain scalar multiplication: one partial sum per proof
            a.nslices = nsc ? 1 : 0;
            part.resize(n * a.nslices);
            for (size_t i = 0; i < n && nsc; i++) {
                JacP acc = JacP::inf();
                for (size_t t = 0; t < nsc; t++) {
                    const Fr x = from_mont(t < nw ? W[i * nw + t] : hashes[i * nc + (t - nw)]);
                    acc = jac_add(acc, g1_mul_words(JacP::from_affine(to_c(vk->K[t + 1])), x.v));
                }
                part[i] = jac_to_xyzz(acc);
            }
            ksum.resize(n);
            folded.resize(nc ? n : 0);
            a.proofs = (const Proof*)proofs;
            a.cmts = cm;
            a.poks = (const G1A*)poks;
            a.K = vk->K.data();
            a.part = part.data();
            a.chal = chal.data();
            a.ksum = ksum.data();
            a.folded = folded.data();
            a.status = status_out;
            a.e = &vk->e;
        }
        a.delta_neg = L;
        a.gamma_neg = L + kLines;
        a.ped_g = L + 2 * kLines;
        a.ped_gs = L + 3 * kLines;
        run(dev, st, Kernels<C>::prep, prep_one, a, n, 64);
        run(dev, st, Kernels<C>::pair, pair_one, a, n, 64);
        if (dev) so.finish(st);
    }
};

}  // namespace groth16v
}  // namespace gg
