// gnark-crypto's point Decoder / Encoder (ecc/<curve>/marshal.go: SetBytes,
// Bytes, RawBytes) for batches of points, for any curve described by a traits
// struct T: point_codec.hip instantiates it for BN254, point_codec_bls.hip for
// BLS12-381.  DESIGN.md §4 "Point codec".
//
// One lane decodes or encodes one point; every step is a per-lane GG_HD
// function that a kernel runs over a grid and the host path over a loop, on the
// same arrays (pairing_run.h: run).
//
//   points side   Montgomery little-endian affine, (0, 0) = infinity: the layout
//                 gg_msm_base_create and the verifiers take
//   bytes side    big-endian canonical coordinates, G2 as X.A1 | X.A0 | Y.A1 | Y.A0,
//                 flags in the top bits of the first byte:
//                 BN254 (2 bits)      00 raw, 01 compressed infinity, 10 / 11
//                                     compressed with y the smaller / larger root;
//                                     the raw infinity is all zero
//                 BLS12-381 (3 bits)  000 raw, 010 raw infinity, 100 / 101
//                                     compressed smaller / larger, 110 compressed
//                                     infinity; 001, 011, 111 invalid
//
// Square roots (both base fields have p = 3 mod 4):
//   Fp    t = a^((p - 3) / 4) by a 4-bit fixed window over the compile-time
//         exponent (pow_p34); the candidate root is t a, checked by squaring
//   Fp2   the complex method through two Fp powers and no inversion.  For
//         a = a0 + a1 u: s = sqrt(a0^2 + a1^2) (s = a0 when a1 = 0), d = (a0 + s) / 2,
//         t = d^((p - 3) / 4), so that t d = d^((p + 1) / 4) and e = t^2 d is the
//         Legendre symbol of d.  e = 1: the root is t d + (a1 t / 2) u (1 / sqrt(d) = t).
//         e = -1: (t d)^2 = -d and (a0 - s) / 2 = -a1^2 / (4 d) = (a1 t / 2)^2, so the
//         root is a1 t / 2 - (t d) u; for a in Fp that is a non-residue this is the
//         purely imaginary branch.  d = 0 only for a = 0.  The result is checked
//         by squaring, which is what refuses the non-squares whose norm has no root.
//
// Status per point (uint8): GG_POINT_OK, GG_POINT_NOT_ON_CURVE (a raw point off
// the curve, a compressed x with no y), GG_POINT_NOT_IN_SUBGROUP, GG_POINT_BAD_ENCODING
// (an invalid flag, a flag that disagrees with the call's encoding, a
// coordinate >= p); a point that is not OK is written as the infinity.
//
// The traits struct T gives
//   Tw            the pairing tower (pairing.cuh)
//   ZCASH         the 3-bit flag layout (else the 2-bit one)
//   g1_member, g2_member   the subgroup test of a point known to be on the curve
#pragma once
#include "common.h"
#include "pairing.cuh"
#include "pairing_run.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace gg {
namespace codec {

using namespace gg::pairing;

constexpr size_t kMaxChunk = (size_t)1 << 20;  // points per launch

// points per launch: 2^20, or GG_CODEC_CHUNK (tests of the chunk loop), in [64, 2^20]
inline size_t chunk_points() {
    size_t c = kMaxChunk;
    if (const char* e = getenv("GG_CODEC_CHUNK")) {
        const long v = atol(e);
        if (v >= 64 && (size_t)v <= kMaxChunk) c = (size_t)v;
    }
    return c;
}

// ---------------------------------------------------------------- field helpers
// word w of (p - 3) / 4 = p >> 2
template <class Cfg>
GG_HD uint32_t p34_word(int w) {
    static_assert((Cfg::P[0] & 3u) == 3u, "p = 3 mod 4");
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) {
        const uint32_t e = (Cfg::P[i] >> 2) | (i + 1 < Cfg::N ? Cfg::P[i + 1] << 30 : 0u);
        r = w == i ? e : r;
    }
    return r;
}
// a^((p - 3) / 4): 4-bit fixed window; the exponent is the same in every lane, so
// no branch diverges.  A call: its three inlined products are the whole body.
template <class Cfg>
GG_HDN Fe<Cfg> pow_p34(const Fe<Cfg>& a) {
    using F = Fe<Cfg>;
    F tab[16];
    tab[0] = F::one();
    tab[1] = a;
#pragma unroll 1
    for (int j = 2; j < 16; j++) tab[j] = tab[j - 1] * a;
    F acc = F::one();
#pragma unroll 1
    for (int w = Cfg::N - 1; w >= 0; w--) {
        const uint32_t word = p34_word<Cfg>(w);
#pragma unroll 1
        for (int s = 28; s >= 0; s -= 4) {
#pragma unroll 1
            for (int k = 0; k < 4; k++) acc = sqr(acc);
            const uint32_t d = (word >> s) & 15u;
            if (d) acc = acc * tab[d];
        }
    }
    return acc;
}
// a / 2 (any representation: halving is linear)
template <class Cfg>
GG_HD Fe<Cfg> half(const Fe<Cfg>& a) {
    const uint32_t m = 0u - (a.v[0] & 1u);
    Fe<Cfg> r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) r.v[i] = __builtin_addc(a.v[i], Cfg::P[i] & m, c, &c);  // < 2^(32 N): p < 2^(32 N - 1)
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) r.v[i] = (r.v[i] >> 1) | (i + 1 < Cfg::N ? r.v[i + 1] << 31 : 0u);
    return r;
}
// the candidate root of a and whether its square is a
template <class Cfg>
GG_HD bool fp_sqrt(const Fe<Cfg>& a, Fe<Cfg>& out) {
    out = pow_p34(a) * a;
    return sqr(out) == a;
}
template <class F2>
GG_HD bool fp2_sqrt(const F2& a, F2& out) {
    using F = decltype(a.a0);
    const bool real = a.a1.is_zero();
    const F n = sqr(a.a0) + sqr(a.a1);
    F s = pow_p34(n) * n;
    if (real) {
        s = a.a0;
    } else if (!(sqr(s) == n)) {  // the norm has no root: a is no square
        out = F2::zero();
        return false;
    }
    const F d = half(a.a0 + s);
    const F t = pow_p34(d);
    const F td = t * d;
    const F h = half(a.a1 * t);
    if (t * td == F::one()) out = F2{td, h};
    else out = F2{h, -td};
    return sqr(out) == a;
}
// LexicographicallyLargest: the canonical value > (p - 1) / 2
template <class Cfg>
GG_HD bool lex_largest(const Fe<Cfg>& mont) {
    const Fe<Cfg> c = from_mont(mont);
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) {
        const uint32_t hw = (Cfg::P[i] >> 1) | (i + 1 < Cfg::N ? Cfg::P[i + 1] << 31 : 0u);
        (void)__builtin_subc(hw, c.v[i], br, &br);
    }
    return br != 0;
}
// E2: compare A1, or A0 when A1 = 0
template <class F2>
GG_HD bool lex_largest2(const F2& y) {
    return lex_largest(y.a1.is_zero() ? y.a0 : y.a1);
}
// big-endian bytes (the first byte under `first_mask`) -> canonical limbs; false when >= p
template <class Cfg>
GG_HD bool load_be(const uint8_t* b, uint8_t first_mask, Fe<Cfg>& out) {
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) {
        const int o = 4 * (Cfg::N - 1 - i);
        const uint32_t b0 = o == 0 ? (uint32_t)(b[0] & first_mask) : (uint32_t)b[o];
        out.v[i] = (b0 << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | (uint32_t)b[o + 3];
    }
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) (void)__builtin_subc(out.v[i], Cfg::P[i], br, &br);
    return br != 0;
}
// Montgomery -> big-endian canonical bytes
template <class Cfg>
GG_HD void store_be(const Fe<Cfg>& mont, uint8_t* b) {
    const Fe<Cfg> c = from_mont(mont);
#pragma unroll
    for (int i = 0; i < Cfg::N; i++) {
        const int o = 4 * (Cfg::N - 1 - i);
        b[o] = (uint8_t)(c.v[i] >> 24);
        b[o + 1] = (uint8_t)(c.v[i] >> 16);
        b[o + 2] = (uint8_t)(c.v[i] >> 8);
        b[o + 3] = (uint8_t)c.v[i];
    }
}

// ---------------------------------------------------------------- per-lane steps
enum Kind { kBad, kRawPoint, kRawInf, kSmall, kLarge, kCompInf };

template <class T>
struct Codec {
    using Tw = typename T::Tw;
    using F = typename Tw::F;
    using F2 = typename Tw::F2;
    using G1A = Affine<F>;
    using G2A = Affine<F2>;
    static constexpr int FB = (int)sizeof(F);  // bytes per coordinate
    static constexpr uint8_t kCoordMask = T::ZCASH ? 0x1f : 0x3f;
    static constexpr uint8_t kFlagSmall = 0x80, kFlagLarge = T::ZCASH ? 0xa0 : 0xc0;
    static constexpr uint8_t kFlagCompInf = T::ZCASH ? 0xc0 : 0x40, kFlagRawInf = T::ZCASH ? 0x40 : 0x00;

    static GG_HD constexpr size_t encoded_size(bool g2, int enc) {
        return (size_t)FB * (g2 ? 2 : 1) * (enc == GG_ENC_RAW ? 2 : 1);
    }
    static GG_HD int classify(uint8_t first) {
        if constexpr (T::ZCASH) {
            switch (first >> 5) {
                case 0: return kRawPoint;
                case 2: return kRawInf;
                case 4: return kSmall;
                case 5: return kLarge;
                case 6: return kCompInf;
                default: return kBad;
            }
        } else {
            switch (first >> 6) {
                case 0: return kRawPoint;
                case 1: return kCompInf;
                case 2: return kSmall;
                default: return kLarge;
            }
        }
    }
    // the flag against the call's encoding: a status, or -1 to go on with a finite point
    static GG_HD int check_flag(int kind, int enc) {
        if (kind == kBad) return GG_POINT_BAD_ENCODING;
        const bool raw_kind = kind == kRawPoint || kind == kRawInf;
        if (raw_kind != (enc == GG_ENC_RAW)) return GG_POINT_BAD_ENCODING;
        if (kind == kRawInf || kind == kCompInf) return GG_POINT_OK;  // the other bytes are not looked at
        return -1;
    }

    static GG_HD int decode_g1(int enc, int flags, const uint8_t* in, G1A& out) {
        out = G1A::inf();
        const int kind = classify(in[0]);
        const int st = check_flag(kind, enc);
        if (st >= 0) return st;
        const bool checks = !(flags & GG_DEC_NO_SUBGROUP_CHECK);
        F x, y;
        if (!load_be(in, kCoordMask, x)) return GG_POINT_BAD_ENCODING;
        if (enc == GG_ENC_RAW) {
            if (!load_be(in + FB, 0xff, y)) return GG_POINT_BAD_ENCODING;
            if (x.is_zero() && y.is_zero()) return GG_POINT_OK;  // the all-zero raw infinity
            x = to_mont(x);
            y = to_mont(y);
            if (checks && !(sqr(y) == sqr(x) * x + Tw::b_g1())) return GG_POINT_NOT_ON_CURVE;
        } else {
            x = to_mont(x);
            if (!fp_sqrt(sqr(x) * x + Tw::b_g1(), y)) return GG_POINT_NOT_ON_CURVE;
            if (lex_largest(y) != (kind == kLarge)) y = -y;
        }
        const G1A p{x, y};
        if (checks && !T::g1_member(p)) return GG_POINT_NOT_IN_SUBGROUP;
        out = p;
        return GG_POINT_OK;
    }
    static GG_HD int decode_g2(int enc, int flags, const uint8_t* in, G2A& out) {
        out = G2A::inf();
        const int kind = classify(in[0]);
        const int st = check_flag(kind, enc);
        if (st >= 0) return st;
        const bool checks = !(flags & GG_DEC_NO_SUBGROUP_CHECK);
        F2 x, y;
        if (!load_be(in, kCoordMask, x.a1)) return GG_POINT_BAD_ENCODING;
        if (!load_be(in + FB, 0xff, x.a0)) return GG_POINT_BAD_ENCODING;
        if (enc == GG_ENC_RAW) {
            if (!load_be(in + 2 * FB, 0xff, y.a1)) return GG_POINT_BAD_ENCODING;
            if (!load_be(in + 3 * FB, 0xff, y.a0)) return GG_POINT_BAD_ENCODING;
            if (x.is_zero() && y.is_zero()) return GG_POINT_OK;
            x = F2{to_mont(x.a0), to_mont(x.a1)};
            y = F2{to_mont(y.a0), to_mont(y.a1)};
            if (checks && !(sqr(y) == sqr(x) * x + Tw::b_twist())) return GG_POINT_NOT_ON_CURVE;
        } else {
            x = F2{to_mont(x.a0), to_mont(x.a1)};
            if (!fp2_sqrt(sqr(x) * x + Tw::b_twist(), y)) return GG_POINT_NOT_ON_CURVE;
            if (lex_largest2(y) != (kind == kLarge)) y = -y;
        }
        const G2A q{x, y};
        if (checks && !T::g2_member(q)) return GG_POINT_NOT_IN_SUBGROUP;
        out = q;
        return GG_POINT_OK;
    }
    static GG_HD void encode_g1(int enc, const G1A& p, uint8_t* out) {
        const int size = (int)encoded_size(false, enc);
        if (p.is_inf()) {
            for (int i = 0; i < size; i++) out[i] = 0;
            out[0] = enc == GG_ENC_RAW ? kFlagRawInf : kFlagCompInf;
            return;
        }
        store_be(p.x, out);
        if (enc == GG_ENC_RAW) store_be(p.y, out + FB);
        else out[0] |= lex_largest(p.y) ? kFlagLarge : kFlagSmall;
    }
    static GG_HD void encode_g2(int enc, const G2A& q, uint8_t* out) {
        const int size = (int)encoded_size(true, enc);
        if (q.is_inf()) {
            for (int i = 0; i < size; i++) out[i] = 0;
            out[0] = enc == GG_ENC_RAW ? kFlagRawInf : kFlagCompInf;
            return;
        }
        store_be(q.x.a1, out);
        store_be(q.x.a0, out + FB);
        if (enc == GG_ENC_RAW) {
            store_be(q.y.a1, out + 2 * FB);
            store_be(q.y.a0, out + 3 * FB);
        } else {
            out[0] |= lex_largest2(q.y) ? kFlagLarge : kFlagSmall;
        }
    }

    struct DecArgs {
        size_t n;
        int enc, flags;
        const uint8_t* in;
        void* out;
        uint8_t* status;
    };
    struct EncArgs {
        size_t n;
        int enc;
        const void* in;
        uint8_t* out;
    };
    struct SqrtArgs {
        size_t n;
        const void* in;
        void* out;
        uint8_t* ok;
    };
    static GG_HD void dec_g1_lane(const DecArgs& a, size_t i) {
        G1A p;
        a.status[i] = (uint8_t)decode_g1(a.enc, a.flags, a.in + i * encoded_size(false, a.enc), p);
        ((G1A*)a.out)[i] = p;
    }
    static GG_HD void dec_g2_lane(const DecArgs& a, size_t i) {
        G2A q;
        a.status[i] = (uint8_t)decode_g2(a.enc, a.flags, a.in + i * encoded_size(true, a.enc), q);
        ((G2A*)a.out)[i] = q;
    }
    static GG_HD void enc_g1_lane(const EncArgs& a, size_t i) {
        encode_g1(a.enc, ((const G1A*)a.in)[i], a.out + i * encoded_size(false, a.enc));
    }
    static GG_HD void enc_g2_lane(const EncArgs& a, size_t i) {
        encode_g2(a.enc, ((const G2A*)a.in)[i], a.out + i * encoded_size(true, a.enc));
    }
    static GG_HD void sqrt1_lane(const SqrtArgs& a, size_t i) {
        F r;
        a.ok[i] = fp_sqrt(((const F*)a.in)[i], r) ? 1 : 0;
        ((F*)a.out)[i] = r;
    }
    static GG_HD void sqrt2_lane(const SqrtArgs& a, size_t i) {
        F2 r;
        a.ok[i] = fp2_sqrt(((const F2*)a.in)[i], r) ? 1 : 0;
        ((F2*)a.out)[i] = r;
    }
};

// the __global__ wrappers, one set per curve (named beside the instantiation)
template <class T>
struct Kernels;

// ---------------------------------------------------------------- host side
// Every entry point walks its n points in chunks of at most chunk_points(): one
// launch per chunk, one bounded wait per chunk, scratch for one chunk.
template <class T>
struct Api {
    using C = Codec<T>;

    static void decode(bool dev, bool g2, int enc, int flags, size_t n, const void* bytes, bool bytes_on_device,
                       void* points_out, bool out_on_device, uint8_t* status_out) {
        const size_t esz = C::encoded_size(g2, enc), psz = g2 ? sizeof(typename C::G2A) : sizeof(typename C::G1A);
        auto kern = g2 ? Kernels<T>::dec_g2 : Kernels<T>::dec_g1;
        auto body = g2 ? C::dec_g2_lane : C::dec_g1_lane;
        if (!dev) {
            const typename C::DecArgs a{n, enc, flags, (const uint8_t*)bytes, points_out, status_out};
            run(false, nullptr, kern, body, a, n, 64);
            return;
        }
        Stream st;
        DevBuf din, dout, dstat;
        const size_t chunk = chunk_points();
        for (size_t off = 0; off < n; off += chunk) {
            const size_t c = n - off < chunk ? n - off : chunk;
            const uint8_t* in = (const uint8_t*)bytes + off * esz;
            if (!bytes_on_device) {
                din.reserve(c * esz);
                GG_HIP(hipMemcpyAsync(din.p, in, c * esz, hipMemcpyHostToDevice, st.s));
                in = din.template as<uint8_t>();
            }
            void* out = (char*)points_out + off * psz;
            if (!out_on_device) {
                dout.reserve(c * psz);
                out = dout.p;
            }
            dstat.reserve(c);
            const typename C::DecArgs a{c, enc, flags, in, out, dstat.template as<uint8_t>()};
            run(true, st.s, kern, body, a, c, 64);
            if (!out_on_device)
                GG_HIP(hipMemcpyAsync((char*)points_out + off * psz, dout.p, c * psz, hipMemcpyDeviceToHost, st.s));
            GG_HIP(hipMemcpyAsync(status_out + off, dstat.p, c, hipMemcpyDeviceToHost, st.s));
            GG_WAIT_STREAM(st.s);
        }
    }
    static void encode(bool dev, bool g2, int enc, size_t n, const void* points, bool points_on_device,
                       void* bytes_out) {
        const size_t esz = C::encoded_size(g2, enc), psz = g2 ? sizeof(typename C::G2A) : sizeof(typename C::G1A);
        auto kern = g2 ? Kernels<T>::enc_g2 : Kernels<T>::enc_g1;
        auto body = g2 ? C::enc_g2_lane : C::enc_g1_lane;
        if (!dev) {
            const typename C::EncArgs a{n, enc, points, (uint8_t*)bytes_out};
            run(false, nullptr, kern, body, a, n, 64);
            return;
        }
        Stream st;
        DevBuf din, dout;
        const size_t chunk = chunk_points();
        for (size_t off = 0; off < n; off += chunk) {
            const size_t c = n - off < chunk ? n - off : chunk;
            const void* in = (const char*)points + off * psz;
            if (!points_on_device) {
                din.reserve(c * psz);
                GG_HIP(hipMemcpyAsync(din.p, in, c * psz, hipMemcpyHostToDevice, st.s));
                in = din.p;
            }
            dout.reserve(c * esz);
            const typename C::EncArgs a{c, enc, in, dout.template as<uint8_t>()};
            run(true, st.s, kern, body, a, c, 64);
            GG_HIP(hipMemcpyAsync((char*)bytes_out + off * esz, dout.p, c * esz, hipMemcpyDeviceToHost, st.s));
            GG_WAIT_STREAM(st.s);
        }
    }
    // in, out, ok: host or device pointers on the device path (pairing_run.h)
    static void sqrt(bool dev, int degree, size_t n, const void* in, void* out, uint8_t* ok) {
        const size_t fsz = sizeof(typename C::F) * (size_t)degree;
        auto kern = degree == 2 ? Kernels<T>::sqrt2 : Kernels<T>::sqrt1;
        auto body = degree == 2 ? C::sqrt2_lane : C::sqrt1_lane;
        if (!dev) {
            const typename C::SqrtArgs a{n, in, out, ok};
            run(false, nullptr, kern, body, a, n, 64);
            return;
        }
        Stream st;
        const size_t chunk = chunk_points();
        for (size_t off = 0; off < n; off += chunk) {
            const size_t c = n - off < chunk ? n - off : chunk;
            DevBuf din;
            OutBuf o, k;
            const void* d = to_device((const char*)in + off * fsz, c * fsz, din, st.s);
            o.init((char*)out + off * fsz, c * fsz);
            k.init(ok + off, c);
            const typename C::SqrtArgs a{c, d, o.dev, (uint8_t*)k.dev};
            run(true, st.s, kern, body, a, c, 64);
            if (o.host) GG_HIP(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, st.s));
            k.finish(st.s);
        }
    }
};

// the kernels of one curve: `name` prefixes them, T is its traits struct
#define GG_CODEC_KERNELS(T, name)                                                                  \
    __global__ void __launch_bounds__(64) name##_dec_g1(Codec<T>::DecArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::dec_g1_lane(a, i);                                                  \
    }                                                                                              \
    __global__ void __launch_bounds__(64) name##_dec_g2(Codec<T>::DecArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::dec_g2_lane(a, i);                                                  \
    }                                                                                              \
    __global__ void __launch_bounds__(64) name##_enc_g1(Codec<T>::EncArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::enc_g1_lane(a, i);                                                  \
    }                                                                                              \
    __global__ void __launch_bounds__(64) name##_enc_g2(Codec<T>::EncArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::enc_g2_lane(a, i);                                                  \
    }                                                                                              \
    __global__ void __launch_bounds__(64) name##_sqrt1(Codec<T>::SqrtArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::sqrt1_lane(a, i);                                                   \
    }                                                                                              \
    __global__ void __launch_bounds__(64) name##_sqrt2(Codec<T>::SqrtArgs a) {                     \
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                            \
        if (i < a.n) Codec<T>::sqrt2_lane(a, i);                                                   \
    }                                                                                              \
    template <>                                                                                    \
    struct Kernels<T> {                                                                            \
        static constexpr auto dec_g1 = name##_dec_g1;                                              \
        static constexpr auto dec_g2 = name##_dec_g2;                                              \
        static constexpr auto enc_g1 = name##_enc_g1;                                              \
        static constexpr auto enc_g2 = name##_enc_g2;                                              \
        static constexpr auto sqrt1 = name##_sqrt1;                                                \
        static constexpr auto sqrt2 = name##_sqrt2;                                                \
    };

// what the C entry points (point_codec.hip) call for BLS12-381 (point_codec_bls.hip)
void bls_decode(bool dev, bool g2, int enc, int flags, size_t n, const void* bytes, bool bytes_on_device,
                void* points_out, bool out_on_device, uint8_t* status_out);
void bls_encode(bool dev, bool g2, int enc, size_t n, const void* points, bool points_on_device, void* bytes_out);
void bls_sqrt(bool dev, int degree, size_t n, const void* in, void* out, uint8_t* ok);

}  // namespace codec
}  // namespace gg
