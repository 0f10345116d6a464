// PlonK Verify for batches of proofs under one verifying key
// (backend/plonk/<curve>/verify.go:45-294) and the plain KZG opening check it is
// made of (kzg.Verify), for any curve described by a traits struct C:
// plonk_verify.hip instantiates it for BN254, plonk_verify_bls.hip for BLS12-381.
//
// Every step is a per-lane GG_HD function; a kernel runs it over a grid and the
// host path over a loop, on the same buffers.
//
//   point_check  lane (item, point): the curve's membership flag of one point
//                (C::kCheckLanes: curves whose test is a scalar multiplication)
//   pi_partial   lane (proof, slice of kPiSlice public inputs): sum L_i(zeta) x_i
//                with one batch inversion (prefix products in a global workspace)
//   fr_phase1    lane per proof: the point checks (or their flags), zeta^n,
//                L_1(zeta), PI(zeta), the quotient identity, the scalars of the two
//                G1 combinations
//   term_mul     lane (item, term): one scalar multiplication, an XYZZ partial
//   group_sum    lane per item: the partials of its two groups -> two affine points
//   pair2        lane per item: e(A, G2) e(B, [tau]G2) == 1, both Miller operands
//                from the key's line tables
//
// Per batch: Fiat-Shamir and the BSB22 hashes on the host; point_check,
// pi_partial, fr_phase1, term_mul, group_sum (foldedH and the linearised digest)
// on the device; the KZG folding challenge and lambda on the host; term_mul,
// group_sum (A and B), pair2 on the device.  DESIGN.md §4 "PlonK Verify".
//
// The traits struct C gives
//   Tw            the pairing tower (pairing.cuh); Tw::F is the stored coordinate
//   Fr            the scalar field
//   PC            the coordinate type of the point loops: Tw::F, or Called<Tw::F>
//                 (the same bytes) where an inlined loop body would outgrow a
//                 short branch
//   kCurve        the GG_CURVE_* id;  kCheckLanes  see point_check
//   P1Extra       base of fr_phase1's arguments: PointFlags with kCheckLanes
//   inv(PC)       the inversion of the affine results
//   g1_flag, g2_flag   0 good, 1 off the curve, 2 outside the r-torsion
//   g1_raw        G1Affine.RawBytes;  hash_to_field  fr.Hash(msg, dst, 1)
// and Kernels<C> (specialised beside the kernels) names the __global__ wrappers.
#pragma once
#include "common.h"
#include "pairing.cuh"
#include "pairing_host.h"
#include "pairing_run.h"
#include "prof.h"
#include "sha256.h"
#include "transcript.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace gg {
namespace plonkv {

using namespace gg::pairing;
constexpr int kPiSlice = 32;  // public inputs per lane of pi_partial
constexpr uint8_t kOk = GG_PLONK_VERIFY_OK;

// the proof's byte layout (gnark_amd.h, gg_plonk_prove): PT-byte points, 32-B fr
template <size_t PT>
struct Layout {
    size_t nc = 0;
    GG_HD size_t n_points() const { return 9 + nc; }
    // LRO 0..2, Z 3, H 4..6, Bsb22 7..7+nc-1, BatchedProof.H 7+nc, ZShiftedOpening.H 8+nc
    GG_HD size_t point(size_t k) const { return k < 8 + nc ? PT * k : zs_h(); }
    GG_HD size_t claimed(size_t j) const { return PT * (8 + nc) + 32 * j; }
    GG_HD size_t zs_h() const { return claimed(7 + nc); }
    GG_HD size_t zu() const { return zs_h() + PT; }
    GG_HD size_t stride() const { return zu() + 32; }
};
// where a term's point lives: 0 = the item's slot of buffer 0 (+ off), 1 = of buffer 1, 2 = the key's points
struct TermSrc {
    uint32_t kind, off;
};
struct NoFlags {};
struct PointFlags {
    const uint8_t* flags = nullptr;  // n x n_points, written by point_check
};

template <class F>
GG_HD const F& at(const uint8_t* base, size_t off) {
    return *reinterpret_cast<const F*>(base + off);
}

template <class C>
struct Kernels;

// a grow-only buffer on either side
struct Buf {
    DevBuf d;
    std::vector<uint8_t> h;
    void* get(bool dev, size_t bytes) {
        if (dev) {
            d.reserve(bytes > 16 ? bytes : 16);
            return d.p;
        }
        if (h.size() < bytes + 16) h.resize(bytes + 16);
        return h.data();
    }
    // the step's view of host data: the data itself, or an upload on st
    const void* in(bool dev, const void* host, size_t bytes, hipStream_t st) {
        if (!dev) return host;
        void* p = get(true, bytes);
        if (bytes) GG_HIP(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, st));
        return p;
    }
};
static void fetch(bool dev, void* host, const void* src, size_t bytes, hipStream_t st) {
    if (dev) {
        GG_HIP(hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
    } else if (host != src) {
        memcpy(host, src, bytes);
    }
}
struct Work {
    Buf proofs, wit, chal, hashes, status, flags, piwork, pipart, scal, part, pts, extra;
};

template <class F>
static bool is_canonical(const F& x) {
    const F m = F::modulus();
    for (int i = (int)(sizeof(F) / 4) - 1; i >= 0; i--)
        if (x.v[i] != m.v[i]) return x.v[i] < m.v[i];
    return false;
}
static const uint8_t kBsb22Dst[] = "BSB22-Plonk";          // verify.go:128
static const uint8_t kLambdaTag[] = "gg-plonk-kzg-lambda";  // the batch-opening coefficient's domain

// The per-proof host work (transcripts, hashes) over [0, n): on kHostThreads
// threads when the hashes are the library's SHA-256; a caller's hash callback
// and its context are not assumed to be thread-safe, so they run on this thread.
constexpr size_t kHostThreads = 8, kHostGrain = 64;
template <class Fn>
static void host_for(size_t n, bool parallel, Fn fn) {
    const size_t nt = parallel ? std::min(kHostThreads, n / kHostGrain) : 0;
    if (nt < 2) {
        for (size_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::mutex emu;
    int code = GG_OK;
    std::string err;
    auto worker = [&](size_t t) {
        try {
            for (size_t i = n * t / nt; i < n * (t + 1) / nt; i++) fn(i);
        } catch (const Error& e) {
            std::lock_guard<std::mutex> g(emu);
            code = e.code;
            err = e.what();
        } catch (const std::exception& e) {
            std::lock_guard<std::mutex> g(emu);
            code = GG_ERR_INTERNAL;
            err = e.what();
        }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back(worker, t);
    worker(0);
    for (auto& x : th) x.join();
    GG_CHECK(code == GG_OK, code, err);
}

template <class C>
struct Verifier {
    using Tw = typename C::Tw;
    using Fr = typename C::Fr;
    using PC = typename C::PC;
    using G1A = Affine<typename Tw::F>;   // as stored
    using G2A = Affine<typename Tw::F2>;
    using G1P = Affine<PC>;               // as the point loops read it
    using XZ = Xyzz<PC>;
    using GT = Fp12<Tw>;
    using LineT = Line<Tw>;
    static constexpr int kLines = line_count<Tw>();
    static constexpr size_t kPt = sizeof(G1A);
    using LayoutT = Layout<kPt>;
    static_assert(sizeof(G1P) == sizeof(G1A) && sizeof(Fr) == 32, "one point layout, 32-byte scalars");

    struct KeyConst {
        uint64_t size = 0, nb_public = 0;
        int log_n = 0;
        uint32_t nc = 0;
        Fr omega, omega_inv, u, size_fr;  // Montgomery
    };
    struct Chal {
        Fr gamma, beta, alpha, zeta;
    };

    // ------------------------------------------------------------ per-lane steps
    struct ChkArgs {
        size_t n, npts;
        const TermSrc* src;  // where point k of an item lives (kinds 0 and 1)
        const uint8_t *b0, *b1;
        size_t s0, s1;
        const uint8_t* status;
        uint8_t* flags;
    };
    static GG_HD void point_check(const ChkArgs& a, size_t id) {
        const size_t p = id / a.npts, k = id - p * a.npts;
        if (a.status[p] != kOk) {  // a coordinate >= p: decided on the host
            a.flags[id] = 0;
            return;
        }
        const TermSrc s = a.src[k];
        const uint8_t* base = s.kind == 0 ? a.b0 + p * a.s0 : a.b1 + p * a.s1;
        a.flags[id] = (uint8_t)C::g1_flag(at<G1A>(base, s.off));
    }

    struct PiArgs {
        KeyConst k;
        size_t n, nslices;
        const Fr* wit;
        const Chal* chal;
        const uint8_t* status;
        Fr* work;  // kPiSlice prefix products per lane
        Fr* part;
    };
    static GG_HD void pi_partial(const PiArgs& a, size_t id) {
        const size_t p = id / a.nslices, s = id - p * a.nslices;
        if (a.status[p] != kOk) return;
        const Fr zeta = a.chal[p].zeta;
        Fr zn = zeta;
        for (int i = 0; i < a.k.log_n; i++) zn = sqr(zn);
        const size_t i0 = s * kPiSlice, i1 = i0 + kPiSlice < a.k.nb_public ? i0 + kPiSlice : a.k.nb_public;
        Fr* pre = a.work + id * kPiSlice;
        // denominators n (zeta - w^i); a zero one stays out of the product and inverts to 0
        Fr acc = Fr::one(), w = pow_u64(a.k.omega, i0);
        for (size_t i = i0; i < i1; i++) {
            pre[i - i0] = acc;
            const Fr d = (zeta - w) * a.k.size_fr;
            if (!d.is_zero()) acc = acc * d;
            w = w * a.k.omega;
        }
        Fr inv = inverse(acc), sum = Fr::zero();
        for (size_t i = i1; i-- > i0;) {
            w = w * a.k.omega_inv;
            const Fr d = (zeta - w) * a.k.size_fr;
            if (!d.is_zero()) {
                sum = sum + w * (inv * pre[i - i0]) * a.wit[p * a.k.nb_public + i];
                inv = inv * d;
            }
        }
        a.part[id] = sum * (zn - Fr::one());
    }

    static GG_HD void store_canonical(uint32_t* out, const Fr& mont) {
        const Fr c = from_mont(mont);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = c.v[i];
    }

    struct P1Args : C::P1Extra {
        KeyConst k;
        LayoutT L;
        size_t n, nslices;
        const uint8_t* proofs;
        const Chal* chal;
        const Fr* hashes;  // n x nc
        const Fr* cmt_w;   // w^(nb_public + commitment_indexes[j])
        const Fr* part;
        uint8_t* status;
        uint32_t* scal;  // n x (10 + nc) canonical scalars
    };
    static GG_HD void fr_phase1(const P1Args& a, size_t p) {
        if (a.status[p] != kOk) return;
        const uint8_t* pr = a.proofs + p * a.L.stride();
        const size_t nc = a.k.nc;
        bool bad = false;
        if constexpr (C::kCheckLanes) {
            for (size_t k = 0; k < a.L.n_points(); k++) bad = bad || a.flags[p * a.L.n_points() + k] != 0;
        } else {
            for (size_t k = 0; k < a.L.n_points(); k++) bad = bad || C::g1_flag(at<G1A>(pr, a.L.point(k))) != 0;
        }
        if (bad) {
            a.status[p] = GG_PLONK_VERIFY_MALFORMED;
            return;
        }
        const Chal c = a.chal[p];
        const Fr one = Fr::one();
        Fr zn = c.zeta;
        for (int i = 0; i < a.k.log_n; i++) zn = sqr(zn);
        const Fr zn1 = zn - one;
        const Fr lag1 = zn1 * inverse((c.zeta - one) * a.k.size_fr);
        Fr pi = Fr::zero();
        for (size_t s = 0; s < a.nslices; s++) pi = pi + a.part[p * a.nslices + s];
        for (size_t j = 0; j < nc; j++) {
            const Fr w = a.cmt_w[j];
            pi = pi + w * zn1 * inverse((c.zeta - w) * a.k.size_fr) * a.hashes[p * nc + j];
        }
        const Fr hq = at<Fr>(pr, a.L.claimed(0)), lin = at<Fr>(pr, a.L.claimed(1)), l = at<Fr>(pr, a.L.claimed(2)),
                 r = at<Fr>(pr, a.L.claimed(3)), o = at<Fr>(pr, a.L.claimed(4)), s1 = at<Fr>(pr, a.L.claimed(5)),
                 s2 = at<Fr>(pr, a.L.claimed(6)), zu = at<Fr>(pr, a.L.zu());
        const Fr v1 = s1 * c.beta + l + c.gamma, v2 = s2 * c.beta + r + c.gamma;
        const Fr a2l = lag1 * c.alpha * c.alpha;  // alpha^2 L_1(zeta)
        const Fr t = v1 * v2 * (o + c.gamma) * c.alpha * zu;
        if (hq != (lin + pi + t - a2l) * inverse(zn1)) {
            a.status[p] = GG_PLONK_VERIFY_QUOTIENT;
            return;
        }
        const Fr zp = zn * sqr(c.zeta);  // zeta^(n + 2)
        const Fr bz = c.beta * c.zeta;
        const Fr a1 = zu * c.beta * v1 * v2 * c.alpha;
        const Fr a2 =
            a2l - (bz + l + c.gamma) * (bz * a.k.u + r + c.gamma) * (bz * sqr(a.k.u) + o + c.gamma) * c.alpha;
        uint32_t* sc = a.scal + p * (10 + nc) * 8;
        store_canonical(sc, one);  // H0, H1, H2
        store_canonical(sc + 8, zp);
        store_canonical(sc + 16, sqr(zp));
        sc += 24;
        for (size_t j = 0; j < nc; j++) store_canonical(sc + 8 * j, at<Fr>(pr, a.L.claimed(7 + j)));  // Bsb22_j
        sc += 8 * nc;
        store_canonical(sc, l);  // Ql Qr Qm Qo Qk S3 Z
        store_canonical(sc + 8, r);
        store_canonical(sc + 16, l * r);
        store_canonical(sc + 24, o);
        store_canonical(sc + 32, one);
        store_canonical(sc + 40, a1);
        store_canonical(sc + 48, a2);
    }

    // k a, k canonical in memory (8 words): double-and-add from the top bit with
    // mixed additions; the doubling is skipped while the accumulator is infinity.
    // Exact for k = 0, 1, k >= 2^253 and a = infinity.
    static GG_HDN XZ g1_mul(const G1P& a, const uint32_t* k) {
        XZ acc = XZ::inf();
        if (a.is_inf()) return acc;
        for (int wd = 7; wd >= 0; wd--) {
            const uint32_t word = k[wd];
            for (int b = 31; b >= 0; b--) {
                if (!acc.is_inf()) acc = xyzz_dbl(acc);
                if ((word >> b) & 1) xyzz_madd_inplace(acc, a);
            }
        }
        return acc;
    }

    struct MulArgs {
        size_t n, T;
        const TermSrc* src;
        const uint8_t *b0, *b1, *key;
        size_t s0, s1;  // bytes per item of b0, b1
        const uint32_t* scal;
        const uint8_t* status;
        XZ* part;
    };
    static GG_HD void term_mul(const MulArgs& a, size_t id) {
        const size_t p = id / a.T, t = id - p * a.T;
        if (a.status[p] != kOk) return;
        const TermSrc s = a.src[t];
        const uint8_t* base = s.kind == 0 ? a.b0 + p * a.s0 : s.kind == 1 ? a.b1 + p * a.s1 : a.key;
        a.part[id] = g1_mul(at<G1P>(base, s.off), a.scal + id * 8);
    }

    static GG_HD G1P xyzz_to_affine(const XZ& p) {
        if (p.is_inf()) return G1P::inf();
        const PC i3 = C::inv(p.zzz);
        return G1P{p.x * sqr(p.zz * i3), p.y * i3};
    }
    struct SumArgs {
        size_t n, T, split;
        bool neg;  // negate the second group's sum
        const uint8_t* status;
        const XZ* part;
        G1P* out;  // [2 p]: sum of terms [0, split), [2 p + 1]: of [split, T)
    };
    static GG_HD void group_sum(const SumArgs& a, size_t p) {
        if (a.status[p] != kOk) return;
        XZ acc = XZ::inf();
        for (size_t t = 0; t < a.split; t++) xyzz_add_inplace(acc, a.part[p * a.T + t]);
        a.out[2 * p] = xyzz_to_affine(acc);
        acc = XZ::inf();
        for (size_t t = a.split; t < a.T; t++) xyzz_add_inplace(acc, a.part[p * a.T + t]);
        const G1P b = xyzz_to_affine(acc);
        a.out[2 * p + 1] = a.neg ? neg(b) : b;
    }

    struct PairArgs {
        size_t n;
        const G1A* pts;        // A, B per item
        const LineT *t0, *t1;  // the lines of G2 and of [tau]G2
        uint8_t* status;
        uint8_t fail;
    };
    static GG_HD void pair2(const PairArgs& a, size_t i) {
        if (a.status[i] != kOk) return;
        G1A p[2];
        G2Src<Tw> s[2];
        p[0] = a.pts[2 * i];
        p[1] = a.pts[2 * i + 1];
        s[0].tab = a.t0;
        s[0].skip = p[0].is_inf();
        s[1].tab = a.t1;
        s[1].skip = p[1].is_inf();
        GT f = GT::one();
        miller_loop<Tw, 2>(f, p, s);
        if (!final_exp(f).is_one()) a.status[i] = a.fail;
    }

    // ------------------------------------------------------------ host side
    static void fr_be(const Fr& mont, uint8_t out[32]) { fs::be_bytes<8>(from_mont(mont).v, out); }
    static bool g1_canonical(const G1A& p) { return is_canonical(p.x) && is_canonical(p.y); }
    static void put_canonical(std::vector<uint32_t>& v, size_t slot, const Fr& mont) {
        const Fr c = from_mont(mont);
        memcpy(&v[8 * slot], c.v, 32);
    }

    // kzg_g2 = {G2, [tau]G2}: checked, then their line tables (2 x kLines)
    static void g2_tables(const void* kzg_g2, std::vector<LineT>& lines) {
        G2A q[2];
        memcpy(q, kzg_g2, sizeof(q));
        for (int t = 0; t < 2; t++) {
            const std::string nm = "kzg_g2[" + std::to_string(t) + "]";
            GG_CHECK(!q[t].is_inf(), GG_ERR_INVALID_ARG, nm + " is the point at infinity");
            GG_CHECK(is_canonical(q[t].x.a0) && is_canonical(q[t].x.a1) && is_canonical(q[t].y.a0) &&
                         is_canonical(q[t].y.a1),
                     GG_ERR_INVALID_ARG, nm + " has a coordinate >= p");
            const int f = C::g2_flag(q[t]);
            GG_CHECK(f != 1, GG_ERR_INVALID_ARG, nm + " is not on the twist");
            GG_CHECK(f == 0, GG_ERR_INVALID_ARG, nm + " is not in the r-torsion");
        }
        lines.resize((size_t)2 * kLines);
        for (int t = 0; t < 2; t++) line_table<Tw>(q[t], lines.data() + (size_t)t * kLines);
    }
    static G1A checked_g1(const void* p, size_t i, const std::string& name) {
        G1A a;
        memcpy(&a, (const uint8_t*)p + kPt * i, kPt);
        const int f = g1_canonical(a) ? C::g1_flag(a) : 1;
        GG_CHECK(f != 1, GG_ERR_INVALID_ARG, name + " is not on the curve");
        GG_CHECK(f == 0, GG_ERR_INVALID_ARG, name + " is not in the r-torsion");
        return a;
    }

    // the membership flags of every item's points, in w.flags (npts per item)
    static uint8_t* check_points(bool dev, hipStream_t st, Work& w, size_t n, size_t npts, const TermSrc* src,
                                 const uint8_t* b0, size_t s0, const uint8_t* b1, size_t s1, const uint8_t* status) {
        ChkArgs c{n, npts, src, b0, b1, s0, s1, status, (uint8_t*)w.flags.get(dev, n * npts)};
        run(dev, st, Kernels<C>::chk, point_check, c, n * npts, 64);
        return c.flags;
    }
    // terms -> partials -> the two group sums of every item, in w.pts (2 affine per item)
    static G1A* combine(bool dev, hipStream_t st, Work& w, size_t n, size_t T, size_t split, bool neg,
                        const TermSrc* src, const uint8_t* b0, size_t s0, const uint8_t* b1, size_t s1,
                        const uint8_t* key, const uint32_t* scal, const uint8_t* status) {
        MulArgs m{n, T, src, b0, b1, key, s0, s1, scal, status, (XZ*)w.part.get(dev, n * T * sizeof(XZ))};
        run(dev, st, Kernels<C>::mul, term_mul, m, n * T, 64);
        SumArgs s{n, T, split, neg, status, m.part, (G1P*)w.pts.get(dev, 2 * n * sizeof(G1P))};
        run(dev, st, Kernels<C>::sum, group_sum, s, n, 64);
        return (G1A*)s.out;
    }

    struct Key {
        KeyConst k;
        LayoutT L;
        std::vector<Fr> cmt_w;
        std::vector<G1A> pts;        // S1 S2 S3 Ql Qr Qm Qo Qk Qcp[nc] G
        std::vector<LineT> lines;    // G2, [tau]G2: kLines each
        std::vector<uint8_t> bound;  // the key's part of the gamma bindings (bindPublicData)
        std::vector<TermSrc> src1, src2, srcc;  // the terms of the two phases, the proof's points
        std::mutex mu;  // one batch at a time per key: the buffers below are the key's
        bool uploaded = false;
        int device = 0;
        hipStream_t st = nullptr;
        DevBuf d_pts, d_lines, d_cmt_w, d_src1, d_src2, d_srcc;
        Work dev, host;
        ~Key() {
            if (st) (void)hipStreamDestroy(st);
        }
    };

    // validates everything and fills *vk; no device call
    static void create_key(Key* vk, uint64_t size, const void* generator, const void* coset_shift, const void* S,
                           const void* Q, const void* Qcp, int n_cmt, const uint32_t* commitment_indexes,
                           size_t nb_public, const void* kzg_g1, const void* kzg_g2) {
        GG_CHECK(generator, GG_ERR_INVALID_ARG, "null argument: generator");
        GG_CHECK(coset_shift, GG_ERR_INVALID_ARG, "null argument: coset_shift");
        GG_CHECK(S, GG_ERR_INVALID_ARG, "null argument: S");
        GG_CHECK(Q, GG_ERR_INVALID_ARG, "null argument: Q");
        GG_CHECK(kzg_g1, GG_ERR_INVALID_ARG, "null argument: kzg_g1");
        GG_CHECK(kzg_g2, GG_ERR_INVALID_ARG, "null argument: kzg_g2");
        GG_CHECK(n_cmt >= 0, GG_ERR_INVALID_ARG, "n_cmt must be >= 0");
        const size_t nc = (size_t)n_cmt;
        GG_CHECK(Qcp || !nc, GG_ERR_INVALID_ARG, "null argument: Qcp");
        GG_CHECK(commitment_indexes || !nc, GG_ERR_INVALID_ARG, "null argument: commitment_indexes");
        GG_CHECK(size >= 2 && !(size & (size - 1)), GG_ERR_INVALID_ARG,
                 "size = " + std::to_string(size) + " must be a power of two >= 2");
        GG_CHECK(nb_public <= size, GG_ERR_INVALID_ARG,
                 "nb_public = " + std::to_string(nb_public) + " exceeds size = " + std::to_string(size));
        for (size_t j = 0; j < nc; j++)
            GG_CHECK(nb_public + commitment_indexes[j] < size, GG_ERR_INVALID_ARG,
                     "commitment index " + std::to_string(commitment_indexes[j]) + " of commitment " +
                         std::to_string(j) + ": nb_public + index >= size = " + std::to_string(size));
        KeyConst& k = vk->k;
        k.size = size;
        k.nb_public = nb_public;
        k.nc = (uint32_t)nc;
        while (((uint64_t)1 << k.log_n) < size) k.log_n++;
        memcpy(&k.omega, generator, 32);
        memcpy(&k.u, coset_shift, 32);
        GG_CHECK(is_canonical(k.omega) && !k.omega.is_zero(), GG_ERR_INVALID_ARG, "generator is zero or >= r");
        GG_CHECK(is_canonical(k.u), GG_ERR_INVALID_ARG, "coset_shift is >= r");
        k.omega_inv = inverse(k.omega);
        k.size_fr = Fr::zero();
        k.size_fr.v[0] = (uint32_t)size;
        k.size_fr.v[1] = (uint32_t)(size >> 32);
        k.size_fr = to_mont(k.size_fr);
        vk->L.nc = nc;
        GG_CHECK(gg_plonk_proof_size_ex(C::kCurve, n_cmt) == vk->L.stride(), GG_ERR_INTERNAL, "proof layout mismatch");
        static const char* qn[5] = {"Ql", "Qr", "Qm", "Qo", "Qk"};
        for (size_t i = 0; i < 3; i++) vk->pts.push_back(checked_g1(S, i, "S[" + std::to_string(i) + "]"));
        for (size_t i = 0; i < 5; i++) vk->pts.push_back(checked_g1(Q, i, qn[i]));
        for (size_t i = 0; i < nc; i++) vk->pts.push_back(checked_g1(Qcp, i, "Qcp[" + std::to_string(i) + "]"));
        vk->pts.push_back(checked_g1(kzg_g1, 0, "kzg_g1"));
        g2_tables(kzg_g2, vk->lines);
        for (size_t j = 0; j < nc; j++) {
            Fr w = Fr::one(), b = k.omega;  // w^(nb_public + index) by square-and-multiply
            for (uint64_t e = nb_public + commitment_indexes[j]; e; e >>= 1) {
                if (e & 1) w = w * b;
                b = sqr(b);
            }
            vk->cmt_w.push_back(w);
        }
        vk->bound.resize(kPt * (8 + nc));
        for (size_t i = 0; i < 8 + nc; i++) C::g1_raw(vk->pts[i], vk->bound.data() + kPt * i);
        // the terms of the two combinations (points: key index i at kPt i)
        const LayoutT& L = vk->L;
        auto proof = [&](size_t point) { return TermSrc{0, (uint32_t)L.point(point)}; };
        auto key = [](size_t i) { return TermSrc{2, (uint32_t)(kPt * i)}; };
        const size_t iG = 8 + nc;
        std::vector<TermSrc>& s1 = vk->src1;  // H0 H1 H2 | Bsb22_j Ql Qr Qm Qo Qk S3 Z
        for (size_t i = 0; i < 3; i++) s1.push_back(proof(4 + i));
        for (size_t j = 0; j < nc; j++) s1.push_back(proof(7 + j));
        for (size_t i = 0; i < 5; i++) s1.push_back(key(3 + i));
        s1.push_back(key(2));
        s1.push_back(proof(3));
        std::vector<TermSrc>& s2 = vk->src2;  // foldedH lin L R O S1 S2 Qcp_j Z G H_b H_z | H_b H_z
        s2.push_back(TermSrc{1, 0});
        s2.push_back(TermSrc{1, (uint32_t)kPt});
        for (size_t i = 0; i < 3; i++) s2.push_back(proof(i));
        s2.push_back(key(0));
        s2.push_back(key(1));
        for (size_t j = 0; j < nc; j++) s2.push_back(key(8 + j));
        s2.push_back(proof(3));
        s2.push_back(key(iG));
        s2.push_back(proof(7 + nc));
        s2.push_back(proof(8 + nc));
        s2.push_back(proof(7 + nc));
        s2.push_back(proof(8 + nc));
        for (size_t i = 0; i < L.n_points(); i++) vk->srcc.push_back(proof(i));
    }

    static void verify_batch(Key* vk, bool dev, size_t n, const void* proofs, const void* public_witness,
                             gg_hash_fn challenge_hash, void* challenge_ctx, gg_hash_fn folding_hash,
                             void* folding_ctx, uint8_t* status_out) {
        GG_CHECK(vk, GG_ERR_INVALID_ARG, "null argument: vk");
        GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
        GG_CHECK(n <= ((size_t)1 << 24), GG_ERR_INVALID_ARG, "n exceeds 2^24 proofs per call");
        GG_CHECK(proofs, GG_ERR_INVALID_ARG, "null argument: proofs");
        GG_CHECK(status_out, GG_ERR_INVALID_ARG, "null argument: status_out");
        const KeyConst& k = vk->k;
        const LayoutT& L = vk->L;
        const size_t nc = k.nc, nw = k.nb_public, stride = L.stride();
        GG_CHECK(public_witness || !nw, GG_ERR_INVALID_ARG, "null argument: public_witness");
        std::lock_guard<std::mutex> lock(vk->mu);
        hipStream_t st = nullptr;
        const uint8_t* key_pts = (const uint8_t*)vk->pts.data();
        const LineT* lines = vk->lines.data();
        const Fr* cmt_w = vk->cmt_w.data();
        const TermSrc *src1 = vk->src1.data(), *src2 = vk->src2.data(), *srcc = vk->srcc.data();
        if (dev) {
            if (!vk->uploaded) {  // the first device batch: the key and its tables
                GG_HIP(hipGetDevice(&vk->device));
                if (!vk->st) GG_HIP(hipStreamCreateWithFlags(&vk->st, hipStreamNonBlocking));
                upload(vk->d_pts, vk->pts.data(), vk->pts.size() * sizeof(G1A), vk->st);
                upload(vk->d_lines, vk->lines.data(), vk->lines.size() * sizeof(LineT), vk->st);
                upload(vk->d_cmt_w, vk->cmt_w.data(), vk->cmt_w.size() * sizeof(Fr), vk->st);
                upload(vk->d_src1, vk->src1.data(), vk->src1.size() * sizeof(TermSrc), vk->st);
                upload(vk->d_src2, vk->src2.data(), vk->src2.size() * sizeof(TermSrc), vk->st);
                if constexpr (C::kCheckLanes)
                    upload(vk->d_srcc, vk->srcc.data(), vk->srcc.size() * sizeof(TermSrc), vk->st);
                GG_WAIT_STREAM(vk->st);
                vk->uploaded = true;
            }
            GG_HIP(hipSetDevice(vk->device));
            st = vk->st;
            key_pts = (const uint8_t*)vk->d_pts.p;
            lines = vk->d_lines.template as<LineT>();
            cmt_w = vk->d_cmt_w.template as<Fr>();
            src1 = vk->d_src1.template as<TermSrc>();
            src2 = vk->d_src2.template as<TermSrc>();
            srcc = vk->d_srcc.template as<TermSrc>();
        }
        Work& w = dev ? vk->dev : vk->host;
        const uint8_t* P = (const uint8_t*)proofs;
        const Fr* W = (const Fr*)public_witness;
        const fs::Hasher ch{challenge_hash, challenge_ctx}, fh{folding_hash, folding_ctx};

        // ---- host: canonical values, gamma beta alpha zeta, the BSB22 hashes
        std::vector<uint8_t> status(n, kOk);
        std::vector<Chal> chal(n);
        std::vector<Fr> hashes(n * nc);
        const bool par = !challenge_hash && !folding_hash;
        host_for(n, par, [&](size_t i) {
            uint8_t b32[32], bp[kPt];
            const uint8_t* pr = P + i * stride;
            bool ok = is_canonical(at<Fr>(pr, L.zu()));
            for (size_t j = 0; j < 7 + nc; j++) ok = ok && is_canonical(at<Fr>(pr, L.claimed(j)));
            for (size_t j = 0; j < nw; j++) ok = ok && is_canonical(W[i * nw + j]);
            for (size_t j = 0; j < L.n_points(); j++) ok = ok && g1_canonical(at<G1A>(pr, L.point(j)));
            if (!ok) {
                status[i] = GG_PLONK_VERIFY_MALFORMED;
                return;
            }
            fs::Transcript<Fr> t({"gamma", "beta", "alpha", "zeta"}, ch);
            t.bind("gamma", vk->bound.data(), vk->bound.size());
            for (size_t j = 0; j < nw; j++) {
                fr_be(W[i * nw + j], b32);
                t.bind("gamma", b32, 32);
            }
            auto bind_pt = [&](const char* name, size_t point) {
                C::g1_raw(at<G1A>(pr, L.point(point)), bp);
                t.bind(name, bp, kPt);
            };
            for (size_t j = 0; j < 3; j++) bind_pt("gamma", j);
            chal[i].gamma = t.compute("gamma");
            chal[i].beta = t.compute("beta");
            for (size_t j = 0; j < nc; j++) bind_pt("alpha", 7 + j);
            bind_pt("alpha", 3);
            chal[i].alpha = t.compute("alpha");
            for (size_t j = 0; j < 3; j++) bind_pt("zeta", 4 + j);
            chal[i].zeta = t.compute("zeta");
            for (size_t j = 0; j < nc; j++) {
                C::g1_raw(at<G1A>(pr, L.point(7 + j)), bp);
                hashes[i * nc + j] = C::hash_to_field(bp, kPt, kBsb22Dst, sizeof(kBsb22Dst) - 1);
            }
        });

        // ---- phase 1: PI(zeta), the quotient identity, foldedH and the linearised digest
        const size_t nslices = (nw + kPiSlice - 1) / kPiSlice, T1 = 10 + nc, T2 = 13 + nc;
        const uint8_t* dP = (const uint8_t*)w.proofs.in(dev, P, n * stride, st);
        const Fr* dW = (const Fr*)w.wit.in(dev, W, n * nw * sizeof(Fr), st);
        const Chal* dC = (const Chal*)w.chal.in(dev, chal.data(), n * sizeof(Chal), st);
        const Fr* dH = (const Fr*)w.hashes.in(dev, hashes.data(), hashes.size() * sizeof(Fr), st);
        uint8_t* dS = (uint8_t*)w.status.get(dev, n);
        if (dev) GG_HIP(hipMemcpyAsync(dS, status.data(), n, hipMemcpyHostToDevice, st));
        else memcpy(dS, status.data(), n);
        std::vector<G1A> fl(2 * n);  // foldedH, linearised digest
        {
            ProfScope prof("plonk_verify_phase1", st, (double)n);
            PiArgs pa{k, n, nslices, dW, dC, dS, (Fr*)w.piwork.get(dev, n * nslices * kPiSlice * sizeof(Fr)),
                      (Fr*)w.pipart.get(dev, n * nslices * sizeof(Fr))};
            run(dev, st, Kernels<C>::pi, pi_partial, pa, n * nslices, 256);
            P1Args p1;
            if constexpr (C::kCheckLanes)
                p1.flags = check_points(dev, st, w, n, L.n_points(), srcc, dP, stride, nullptr, 0, dS);
            p1.k = k;
            p1.L = L;
            p1.n = n;
            p1.nslices = nslices;
            p1.proofs = dP;
            p1.chal = dC;
            p1.hashes = dH;
            p1.cmt_w = cmt_w;
            p1.part = pa.part;
            p1.status = dS;
            p1.scal = (uint32_t*)w.scal.get(dev, n * T2 * 32);
            run(dev, st, Kernels<C>::fr, fr_phase1, p1, n, 256);
            const G1A* o =
                combine(dev, st, w, n, T1, 3, false, src1, dP, stride, nullptr, 0, key_pts, p1.scal, dS);
            if (dev) GG_HIP(hipMemcpyAsync(fl.data(), o, 2 * n * sizeof(G1A), hipMemcpyDeviceToHost, st));
            else memcpy(fl.data(), o, 2 * n * sizeof(G1A));
            fetch(dev, status.data(), dS, n, st);
            prof.stop(st);
        }

        // ---- host: the KZG folding challenge, lambda, the scalars of A and B
        std::vector<uint32_t> scal(n * T2 * 8, 0);
        host_for(n, par, [&](size_t i) {
            if (status[i] != kOk) return;
            uint8_t b32[32], bp[kPt];
            const uint8_t* pr = P + i * stride;
            const Fr zeta = chal[i].zeta, zu = at<Fr>(pr, L.zu());
            fs::Transcript<Fr> t({"gamma"}, fh);
            fr_be(zeta, b32);
            t.bind("gamma", b32, 32);
            auto bind_g1 = [&](const G1A& p) {
                C::g1_raw(p, bp);
                t.bind("gamma", bp, kPt);
            };
            bind_g1(fl[2 * i]);
            bind_g1(fl[2 * i + 1]);
            for (size_t j = 0; j < 3; j++) bind_g1(at<G1A>(pr, L.point(j)));
            bind_g1(vk->pts[0]);
            bind_g1(vk->pts[1]);
            for (size_t j = 0; j < nc; j++) bind_g1(vk->pts[8 + j]);
            for (size_t j = 0; j < 7 + nc; j++) {
                fr_be(at<Fr>(pr, L.claimed(j)), b32);
                t.bind("gamma", b32, 32);
            }
            fr_be(zu, b32);
            t.bind("gamma", b32, 32);
            const Fr gk = t.compute("gamma");
            // lambda = SHA-256(tag | gk | RawBytes(BatchedProof.H) | RawBytes(ZShiftedOpening.H)) mod r, 0 -> 1
            Sha256 sh;
            sh.update(kLambdaTag, sizeof(kLambdaTag) - 1);
            fr_be(gk, b32);
            sh.update(b32, 32);
            C::g1_raw(at<G1A>(pr, L.point(7 + nc)), bp);
            sh.update(bp, kPt);
            C::g1_raw(at<G1A>(pr, L.point(8 + nc)), bp);
            sh.update(bp, kPt);
            sh.final(b32);
            Fr lambda = fs::fr_set_bytes<Fr>(b32, 32);
            if (lambda.is_zero()) lambda = Fr::one();
            // A: gk^j D_j (7 + nc digests), lambda Z, -(sum gk^j y_j + lambda zu) G, zeta H_b, lambda zeta w H_z
            // B: H_b, lambda H_z (negated by the sum)
            const size_t s0 = i * T2;
            Fr g = Fr::one(), fy = Fr::zero();
            for (size_t j = 0; j < 7 + nc; j++) {
                put_canonical(scal, s0 + j, g);
                fy = fy + g * at<Fr>(pr, L.claimed(j));
                g = g * gk;
            }
            put_canonical(scal, s0 + 7 + nc, lambda);
            put_canonical(scal, s0 + 8 + nc, -(fy + lambda * zu));
            put_canonical(scal, s0 + 9 + nc, zeta);
            put_canonical(scal, s0 + 10 + nc, lambda * zeta * k.omega);
            put_canonical(scal, s0 + 11 + nc, Fr::one());
            put_canonical(scal, s0 + 12 + nc, lambda);
        });

        // ---- phase 2: A, B and e(A, G2) e(B, [tau]G2) == 1
        {
            ProfScope prof("plonk_verify_phase2", st, (double)n);
            const uint8_t* dE = (const uint8_t*)w.extra.in(dev, fl.data(), 2 * n * sizeof(G1A), st);
            const uint32_t* dSc = (const uint32_t*)w.scal.in(dev, scal.data(), scal.size() * 4, st);
            const G1A* ab = combine(dev, st, w, n, T2, 11 + nc, true, src2, dP, stride, dE, 2 * sizeof(G1A), key_pts,
                                    dSc, dS);
            PairArgs pa{n, ab, lines, lines + kLines, dS, GG_PLONK_VERIFY_KZG};
            run(dev, st, Kernels<C>::pair, pair2, pa, n, 64);
            fetch(dev, status_out, dS, n, st);
            prof.stop(st);
        }
    }

    // kzg.Verify of n openings: A_i = C_i - y_i G + z_i H_i, B_i = -H_i, through
    // the PlonK path's term_mul / group_sum / pair2
    static void kzg_verify(bool dev, size_t n, const void* kzg_g1, const void* kzg_g2, const void* digests,
                           const void* quotients, const void* points, const void* values, uint8_t* ok_out) {
        GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
        GG_CHECK(n <= ((size_t)1 << 24), GG_ERR_INVALID_ARG, "n exceeds 2^24 openings per call");
        GG_CHECK(kzg_g1, GG_ERR_INVALID_ARG, "null argument: kzg_g1");
        GG_CHECK(kzg_g2, GG_ERR_INVALID_ARG, "null argument: kzg_g2");
        GG_CHECK(digests, GG_ERR_INVALID_ARG, "null argument: digests");
        GG_CHECK(quotients, GG_ERR_INVALID_ARG, "null argument: quotients");
        GG_CHECK(points, GG_ERR_INVALID_ARG, "null argument: points");
        GG_CHECK(values, GG_ERR_INVALID_ARG, "null argument: values");
        GG_CHECK(ok_out, GG_ERR_INVALID_ARG, "null argument: ok_out");
        const G1A g = checked_g1(kzg_g1, 0, "kzg_g1");
        std::vector<LineT> lines;
        g2_tables(kzg_g2, lines);
        const G1A *Cm = (const G1A*)digests, *H = (const G1A*)quotients;
        const Fr *Z = (const Fr*)points, *Y = (const Fr*)values;
        // C x 1, G x -y, H x z | H x 1; a scalar or a coordinate that is not reduced: rejected here; a
        // point off the curve or outside the subgroup: here, or by the point_check lanes (kCheckLanes)
        const TermSrc src[6] = {{0, 0}, {2, 0}, {1, 0}, {1, 0}, /* the points to check */ {0, 0}, {1, 0}};
        std::vector<uint8_t> status(n, 0);
        std::vector<uint32_t> scal(n * 4 * 8, 0);
        for (size_t i = 0; i < n; i++) {
            bool ok = g1_canonical(Cm[i]) && g1_canonical(H[i]) && is_canonical(Z[i]) && is_canonical(Y[i]);
            if constexpr (!C::kCheckLanes) ok = ok && C::g1_flag(Cm[i]) == 0 && C::g1_flag(H[i]) == 0;
            if (!ok) {
                status[i] = 1;
                continue;
            }
            put_canonical(scal, 4 * i, Fr::one());
            put_canonical(scal, 4 * i + 1, -Y[i]);
            put_canonical(scal, 4 * i + 2, Z[i]);
            put_canonical(scal, 4 * i + 3, Fr::one());
        }
        Work w;
        hipStream_t st = nullptr;
        struct StreamGuard {
            hipStream_t s = nullptr;
            ~StreamGuard() {
                if (s) (void)hipStreamDestroy(s);
            }
        } sg;
        DevBuf d_lines, d_g, d_src;
        const LineT* L = lines.data();
        const uint8_t* key = (const uint8_t*)&g;
        const TermSrc* dsrc = src;
        if (dev) {
            GG_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
            st = sg.s;
            upload(d_lines, lines.data(), lines.size() * sizeof(LineT), st);
            upload(d_g, &g, sizeof(g), st);
            upload(d_src, src, sizeof(src), st);
            L = d_lines.template as<LineT>();
            key = (const uint8_t*)d_g.p;
            dsrc = d_src.template as<TermSrc>();
        }
        const uint8_t* dC = (const uint8_t*)w.proofs.in(dev, Cm, n * kPt, st);
        const uint8_t* dH = (const uint8_t*)w.extra.in(dev, H, n * kPt, st);
        const uint32_t* dSc = (const uint32_t*)w.scal.in(dev, scal.data(), scal.size() * 4, st);
        uint8_t* dS = (uint8_t*)const_cast<void*>(w.status.in(dev, status.data(), n, st));
        std::vector<uint8_t> flags;
        if constexpr (C::kCheckLanes) {
            // the flags come back with the verdicts: a point they reject has gone through the
            // arithmetic below (field operations on its coordinates), and its verdict is dropped
            const uint8_t* dF = check_points(dev, st, w, n, 2, dsrc + 4, dC, kPt, dH, kPt, dS);
            flags.resize(2 * n);
            if (dev) GG_HIP(hipMemcpyAsync(flags.data(), dF, 2 * n, hipMemcpyDeviceToHost, st));
            else memcpy(flags.data(), dF, 2 * n);
        }
        const G1A* ab = combine(dev, st, w, n, 4, 3, true, dsrc, dC, kPt, dH, kPt, key, dSc, dS);
        PairArgs pa{n, ab, L, L + kLines, dS, 1};
        run(dev, st, Kernels<C>::pair, pair2, pa, n, 64);
        fetch(dev, status.data(), dS, n, st);
        for (size_t i = 0; i < n; i++) {
            bool ok = status[i] == 0;
            if constexpr (C::kCheckLanes) ok = ok && !flags[2 * i] && !flags[2 * i + 1];
            ok_out[i] = ok ? 1 : 0;
        }
    }
};

}  // namespace plonkv
}  // namespace gg
