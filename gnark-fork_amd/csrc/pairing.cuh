// Pairing engine for BN254 (optimal ate), host + device: the Fp12 tower over
// Fp2, the multi-Miller loop with projective line functions, the final
// exponentiation, and the G1 / G2 membership checks that Groth16 Verify needs
// (backend/groth16/bn254/verify.go:43-140).
//
// Tower: Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v), xi = 9 + u, so
// w^6 = xi.  The struct layout IS gnark-crypto's E12 memory layout
// (C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2, each an E2 {A0, A1} in
// Montgomery form, 384 B); in the basis sum c_i w^i that order is
// c0, c2, c4, c1, c3, c5.
//
// Untwist (D-type): (x, y) on the twist -> (x w^2, y w^3).  The line through
// T (and Q) evaluated at P = (xp, yp) is a yp + b xp w + c w^3 with a, b, c in
// Fp2; common Fp2 factors are left in (the final exponentiation kills them), so
// the steps need no inversion:
//   doubling (Jacobian, dbl-2009-l):  a = Z3 Z^2, b = -3 X^2 Z^2, c = 3 X^3 - 2 Y^2
//   mixed addition (Z3 = Z H):        a = Z3,     b = -r,         c = r x2 - Z3 y2
// The three coefficients of a FIXED G2 operand are computed once
// (line_table) and read back in the loop.
//
// Final exponentiation: easy part (p^6 - 1)(p^2 + 1), then the hard part of
// Fuentes-Castaneda, Knapp, Rodriguez-Henriquez (SAC 2011): the result is
//   e(P, Q)^m,  m = 2 x (6 x^2 + 3 x + 1),  x = 4965661367192848881,
// the same multiple gnark-crypto's chain computes; gcd(m, r) = 1.
// m = 1469306990098747947464455738335385361638823152381947992820.
//
// Everything is templated on a tower description: Bn254Tower, and beside it
// Bls12381Tower over Fp2Bls (its own comment below says what differs: the twist
// type and the line positions, the loop, the hard part).  The Fp12-level routines are
// not inlined: one lane computes one product of pairings and keeps f in its
// stack frame ("Groth16 Verify").
#pragma once
#include "curve.cuh"

#define GG_HDN __host__ __device__ __attribute__((noinline))

namespace gg {
namespace pairing {

struct Bn254Tower {
    using F = Fp;
    using F2 = Fp2;
    // the group order r, 64-bit words
    static constexpr uint64_t R0 = 0x43e1f593f0000001ull, R1 = 0x2833e84879b97091ull, R2 = 0xb85045b68181585dull,
                              R3 = 0x30644e72e131a029ull;
    static constexpr uint64_t X = 0x44e992b44a6909f1ull;        // the curve's parameter, 63 bits
    static constexpr uint64_t LOOP_LO = 0x9d797039be763ba8ull;  // 6x + 2 = 2^64 + LOOP_LO
    static constexpr int LOOP_STEPS = 64;     // loop bits below the top bit of 6x + 2
    static constexpr int X_TOP = 62;          // the top bit of x
    static constexpr bool X_NEGATIVE = false;
    static constexpr bool M_TWIST = false;    // D-type: lines at w^0, w^1, w^3
    static constexpr bool FROBENIUS_LINES = true;
    static constexpr bool HARD_PART_BLS12 = false;
    static constexpr bool G1_COFACTOR_ONE = true;
    static constexpr bool CALLED_POINT_OPS = false;  // times_r_is_inf: products inlined
    static constexpr int NL = sizeof(F) / 4;  // limbs per Fp coordinate
    // xi^(i (p^1 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G1C[5][16] = {
    {0x33144907u, 0xaf9ba696u, 0x87afb78au, 0xca6b1d73u, 0xf08a2087u, 0x11bded5eu, 0x1a1f3a7cu, 0x02f34d75u,
     0x4c492d72u, 0xa222ae23u, 0x565de15bu, 0xd00f02a4u, 0x53dfc926u, 0xdc2ff3a2u, 0xb3899551u, 0x10a75716u},
    {0x4563ab30u, 0xb5773b10u, 0xa9aa6454u, 0x347f91c8u, 0x242e0991u, 0x7a007127u, 0x118214ecu, 0x1956bcd8u,
     0xa0aa4757u, 0x6e849f1eu, 0x89f89141u, 0xaa1c7b6du, 0xfae0ca3au, 0xb6e713cdu, 0x4e82ebc3u, 0x26694fbbu},
    {0x2936b629u, 0xe4bbdd0cu, 0xe133bacbu, 0xbb30f162u, 0xf9645366u, 0x31a9d1b6u, 0xa500f8ddu, 0x253570beu,
     0x5ffe77c7u, 0xa1d77ce4u, 0x7826d1dbu, 0x07affd11u, 0xbb7edc6bu, 0x6d16bd27u, 0x85defeccu, 0x2c872002u},
    {0x843abe92u, 0x7361d77fu, 0x273411fbu, 0xa5bb2bd3u, 0x4b3e2399u, 0x9c941f31u, 0xbb9fd3ecu, 0x15df9cddu,
     0x4bd8c949u, 0x5dddfd15u, 0xa4445b60u, 0x62cb29a5u, 0x0c7dd2b9u, 0x37bc870au, 0x3171f0fdu, 0x24830a9du},
    {0x41690fe7u, 0xc970692fu, 0x27694b0bu, 0xe2403421u, 0x83c459e8u, 0x32bee66bu, 0x0ab08841u, 0x12aabcedu,
     0x40aebfa9u, 0x0d485d23u, 0xab2fcc57u, 0x05193418u, 0x8a4910f5u, 0xd3b0a40bu, 0x35d2925au, 0x2f21ebb5u}};
    // xi^(i (p^2 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G2C[5][16] = {
    {0x00fa1bf2u, 0xca8d8005u, 0x68b39769u, 0xf0c5d614u, 0xad0d4418u, 0x0e201271u, 0xbad856e6u, 0x04290f65u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x13e80b9cu, 0x3350c88eu, 0xdb5e56b9u, 0x7dce557cu, 0xb615564au, 0x6001b4b8u, 0x020217e0u, 0x2682e617u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x12edefaau, 0x68c34889u, 0x72aabf4fu, 0x8d087f68u, 0x09081231u, 0x51e1a247u, 0x4729c0fau, 0x2259d6b1u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xc494f1abu, 0x08cfc388u, 0x8d1373d4u, 0x19b31514u, 0xcb6c0213u, 0x584e90fdu, 0xdf2f8849u, 0x09e1685bu,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}};
    // xi^(i (p^3 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G3C[5][16] = {
    {0x4e46d97du, 0x36531618u, 0xd4c96d9fu, 0x0af7129eu, 0xca1009b5u, 0x659da72fu, 0x83a20d23u, 0x08116d89u,
     0xc39c1939u, 0xb1df4af7u, 0x8a73bf7fu, 0x3d9f0287u, 0x8caf0ae0u, 0x9b222092u, 0xeff054a6u, 0x26684515u},
    {0x16ad6badu, 0xc9af22f7u, 0x4aa662b2u, 0xb311782au, 0xe248c7f4u, 0x19eeaf64u, 0xe3439f82u, 0x20273e77u,
     0xf7ce93acu, 0xacc02860u, 0x7ba76b4cu, 0x3933d581u, 0x446c8467u, 0x69e6188bu, 0x4417cc55u, 0x0a46036du},
    {0xaf46471eu, 0x5764af0au, 0x873e0fc1u, 0xdc50792eu, 0x881d04f6u, 0x86a673ffu, 0x3c30a74cu, 0x0b2eddb4u,
     0x787e8580u, 0x9a490f32u, 0xf04af8b1u, 0x8fd16d7fu, 0xc6027bf2u, 0x4b39888eu, 0x5b52a15du, 0x03dd2e70u},
    {0x7b6762dfu, 0x448a93a5u, 0x28fdeadfu, 0xbfd62df5u, 0x0e9bd47au, 0xd858f5d0u, 0x3476ec58u, 0x06b03d4du,
     0xbcc936d1u, 0x2b19daf4u, 0x56f4299fu, 0xa1a54e7au, 0x5adeaef1u, 0xb533eee0u, 0x84dda0b2u, 0x170c812bu},
    {0x75cf559fu, 0xe0bc4b22u, 0xc154e60fu, 0xc238b945u, 0x929a7d5eu, 0x803982a5u, 0xf7e4a37eu, 0x15ce052du,
     0xbf3799a7u, 0x2d28efbdu, 0x1ad60773u, 0x9b097e3cu, 0xaf4a535bu, 0x982d4113u, 0xe3056063u, 0x24e18991u}};
    // twist coefficient b' = 3 / xi
    static constexpr uint32_t BT[16] =
    {0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u,
     0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu};
    // xi^(I (p^K - 1) / 6) and b', read limb by limb so that device code folds the constants
    template <int K, int I>
    static GG_HD F2 gamma() {
        F2 r;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            r.a0.v[i] = K == 1 ? G1C[I - 1][i] : K == 2 ? G2C[I - 1][i] : G3C[I - 1][i];
            r.a1.v[i] = K == 1 ? G1C[I - 1][NL + i] : K == 2 ? G2C[I - 1][NL + i] : G3C[I - 1][NL + i];
        }
        return r;
    }
    static GG_HD F2 b_twist() {
        F2 r;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            r.a0.v[i] = BT[i];
            r.a1.v[i] = BT[NL + i];
        }
        return r;
    }
    // a (9 + u)
    static GG_HD F2 mul_xi(const F2& a) {
        F2 t = dbl(dbl(dbl(a))) + a;
        return F2{t.a0 - a.a1, t.a1 + a.a0};
    }
    static GG_HD F2 conj(const F2& a) { return F2{a.a0, -a.a1}; }
    static GG_HD F2 scale(const F2& a, const F& s) { return F2{a.a0 * s, a.a1 * s}; }
    static GG_HD F b_g1() {  // 3
        F o = F::one();
        return o + o + o;
    }
};

// BLS12-381 (ate): Fp2 = Fp[u]/(u^2 + 1), xi = 1 + u, the same tower shape and
// E12 memory layout (576 B).  G1: y^2 = x^3 + 4; the twist is M-type,
// y^2 = x^3 + 4 xi, untwisted by (x, y) -> (x / w^2, y / w^3).  The line through
// T at P = (xp, yp), scaled by w^3 (in Fp4: the final exponentiation kills it),
// is c + b xp w^2 + a yp w^3 with the SAME a, b, c as above: only the
// positions change (w^0, w^2, w^3 = C0.B0, C0.B1, C1.B1).
// x = -0xd201000000010000: the loop runs over |x| (64 bits, weight 6: 63
// doublings + 5 additions = 68 lines), no Frobenius lines, one conjugation.
// Hard part (Hayashida, Hayasaka, Teruya):
//   3 Phi_12(p) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3,
// so the result is e(P, Q)^3; gcd(3, r) = 1.  Whether gnark-crypto's
// FinalExponentiation yields the same bytes: parity unpinned.
// Tables: tools/gen_bls12_381_tower.py.
struct Bls12381Tower {
    using F = FpBls;
    using F2 = Fp2Bls;
    // the group order r (255 bits), 64-bit words
    static constexpr uint64_t R0 = 0xffffffff00000001ull, R1 = 0x53bda402fffe5bfeull, R2 = 0x3339d80809a1d805ull,
                              R3 = 0x73eda753299d7d48ull;
    static constexpr uint64_t X = 0xd201000000010000ull;        // |x|, 64 bits
    static constexpr uint64_t LOOP_LO = 0x5201000000010000ull;  // |x| = 2^63 + LOOP_LO
    static constexpr int LOOP_STEPS = 63;
    static constexpr int X_TOP = 63;
    static constexpr bool X_NEGATIVE = true;
    static constexpr bool M_TWIST = true;     // lines at w^0, w^2, w^3
    static constexpr bool FROBENIUS_LINES = false;
    static constexpr bool HARD_PART_BLS12 = true;
    static constexpr bool G1_COFACTOR_ONE = false;
    static constexpr bool CALLED_POINT_OPS = true;   // times_r_is_inf: products as calls (see there)
    static constexpr int NL = sizeof(F) / 4;
    // xi^(i (p^1 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G1C[5][24] = {
    {0xb319d465u, 0x07089552u, 0xb50a8313u, 0xc6695f92u, 0xd117228fu, 0x97e83cccu, 0xb2dc29eeu, 0xa35baecau,
     0x5daace4du, 0x1ce393eau, 0xb0fb66ebu, 0x08f2220fu, 0x4ce5d646u, 0xb2f66aadu, 0xfc497cecu, 0x5842a06bu,
     0x2599d394u, 0xcf4895d4u, 0x40a8e8d0u, 0xc11b9cbau, 0xe5a0de89u, 0x2e3813cbu, 0x88847fafu, 0x110eefdau},
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u,
     0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u},
    {0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u,
     0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu, 0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u,
     0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu},
    {0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu,
     0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x0dbce43fu, 0x82d83cf5u, 0xdf9d018fu, 0xa2813e53u, 0x3c65e181u, 0xc6f0caa5u, 0x8d50fe95u, 0x7525cf52u,
     0xf4798a6bu, 0x4a85ed50u, 0x6cf8eebdu, 0x171da0fdu, 0xf242c66cu, 0x3726c30au, 0xd1b6fe70u, 0x7c2ac1aau,
     0xba4b14a2u, 0xa04007fbu, 0x66341429u, 0xef517c32u, 0x4ed2226bu, 0x0095ba65u, 0xcc86f7ddu, 0x02e370ecu}};
    // xi^(i (p^2 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G2C[5][24] = {
    {0x798dba3au, 0xecfb361bu, 0x91865a2cu, 0xc100ddb8u, 0x232bda8eu, 0x0ec08ff1u, 0xf1ca4721u, 0xd5c13cc6u,
     0xbf7b5c04u, 0x47222a47u, 0xe51c5f59u, 0x0110f184u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au, 0x74fd029bu, 0xc26a2ff8u,
     0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xfffcaaaeu, 0x43f5ffffu, 0xed47fffdu, 0x32b7fff2u, 0xa2e99d69u, 0x07e83a49u, 0x8332bb7au, 0xeca8f331u,
     0xa0f4c069u, 0xef148d1eu, 0x3eff0206u, 0x040ab326u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu,
     0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu,
     0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}};
    // xi^(i (p^3 - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs
    static constexpr uint32_t G3C[5][24] = {
    {0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du, 0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu,
     0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu, 0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u,
     0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu},
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x0002fffdu, 0x76090000u, 0xc40c0002u, 0xebf4000bu,
     0x53c758bau, 0x5f489857u, 0x70525745u, 0x77ce5853u, 0xa256ec6du, 0x5c071a97u, 0xfa80e493u, 0x15f65ec3u},
    {0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du, 0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu,
     0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu, 0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du,
     0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu, 0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu},
    {0xfffcaaaeu, 0x43f5ffffu, 0xed47fffdu, 0x32b7fff2u, 0xa2e99d69u, 0x07e83a49u, 0x8332bb7au, 0xeca8f331u,
     0xa0f4c069u, 0xef148d1eu, 0x3eff0206u, 0x040ab326u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u, 0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u,
     0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu, 0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du,
     0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu, 0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu}};
    // twist coefficient b' = 4 xi
    static constexpr uint32_t BT[24] =
    {0x000cfff3u, 0xaa270000u, 0xfc34000au, 0x53cc0032u, 0x6b0a807fu, 0x478fe97au, 0xe6ba24d7u, 0xb1d37ebeu,
     0xbf78ab2fu, 0x8ec9733bu, 0x3d83de7eu, 0x09d64551u, 0x000cfff3u, 0xaa270000u, 0xfc34000au, 0x53cc0032u,
     0x6b0a807fu, 0x478fe97au, 0xe6ba24d7u, 0xb1d37ebeu, 0xbf78ab2fu, 0x8ec9733bu, 0x3d83de7eu, 0x09d64551u};
    // phi(x, y) = (BETA x, y): [x^2] phi(P) + P = 0 on G1
    static constexpr uint32_t BETA[12] =
    {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu,
     0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
    // psi(x, y) = (conj(x) PSI[0], conj(y) PSI[1]): psi(Q) = [x] Q on G2
    static constexpr uint32_t PSI[2][24] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u,
     0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u, 0x14e4f04fu, 0x1564853au, 0x14e56d3fu},
    {0xa55c9ad1u, 0x3e2f585du, 0x86c18183u, 0x4294213du, 0x8b623732u, 0x382844c8u, 0x19103e18u, 0x92ad2afdu,
     0xac7cf0b9u, 0x1d794e4fu, 0x7d825ec8u, 0x0bd592fcu, 0x5aa30fdau, 0x7bcfa7a2u, 0x2a927e7cu, 0xdc17dec1u,
     0x6b4ebef1u, 0x2f088dd8u, 0xda74d4a7u, 0xd1ca2087u, 0x96cebc1du, 0x2da25966u, 0xbbfd87d2u, 0x0e2b7eedu}};
    template <int K, int I>
    static GG_HD F2 gamma() {
        F2 r;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            r.a0.v[i] = K == 1 ? G1C[I - 1][i] : K == 2 ? G2C[I - 1][i] : G3C[I - 1][i];
            r.a1.v[i] = K == 1 ? G1C[I - 1][NL + i] : K == 2 ? G2C[I - 1][NL + i] : G3C[I - 1][NL + i];
        }
        return r;
    }
    static GG_HD F2 b_twist() {
        F2 r;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            r.a0.v[i] = BT[i];
            r.a1.v[i] = BT[NL + i];
        }
        return r;
    }
    static GG_HD F endo_beta() {
        F r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.v[i] = BETA[i];
        return r;
    }
    template <int I>
    static GG_HD F2 endo_psi() {
        F2 r;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            r.a0.v[i] = PSI[I][i];
            r.a1.v[i] = PSI[I][NL + i];
        }
        return r;
    }
    // a (1 + u)
    static GG_HD F2 mul_xi(const F2& a) { return F2{a.a0 - a.a1, a.a0 + a.a1}; }
    static GG_HD F2 conj(const F2& a) { return F2{a.a0, -a.a1}; }
    static GG_HD F2 scale(const F2& a, const F& s) { return F2{a.a0 * s, a.a1 * s}; }
    static GG_HD F b_g1() {  // 4
        const F t = F::one() + F::one();
        return t + t;
    }
};

template <class Tw>
struct Fp6 {
    typename Tw::F2 b0, b1, b2;
};
template <class Tw>
struct Fp12 {
    Fp6<Tw> c0, c1;
    static GG_HD Fp12 one() {
        using F2 = typename Tw::F2;
        return Fp12{{F2::one(), F2::zero(), F2::zero()}, {F2::zero(), F2::zero(), F2::zero()}};
    }
    GG_HD bool operator==(const Fp12& o) const {
        return c0.b0 == o.c0.b0 && c0.b1 == o.c0.b1 && c0.b2 == o.c0.b2 && c1.b0 == o.c1.b0 && c1.b1 == o.c1.b1 &&
               c1.b2 == o.c1.b2;
    }
    GG_HD bool is_one() const { return *this == one(); }
};

// ---------------------------------------------------------------- Fp6
template <class Tw>
GG_HD Fp6<Tw> operator+(const Fp6<Tw>& a, const Fp6<Tw>& b) {
    return Fp6<Tw>{a.b0 + b.b0, a.b1 + b.b1, a.b2 + b.b2};
}
template <class Tw>
GG_HD Fp6<Tw> operator-(const Fp6<Tw>& a, const Fp6<Tw>& b) {
    return Fp6<Tw>{a.b0 - b.b0, a.b1 - b.b1, a.b2 - b.b2};
}
template <class Tw>
GG_HD Fp6<Tw> operator-(const Fp6<Tw>& a) {
    return Fp6<Tw>{-a.b0, -a.b1, -a.b2};
}
// a v
template <class Tw>
GG_HD Fp6<Tw> mul_v(const Fp6<Tw>& a) {
    return Fp6<Tw>{Tw::mul_xi(a.b2), a.b0, a.b1};
}
// Karatsuba, 6 Fp2 products
template <class Tw>
GG_HDN Fp6<Tw> operator*(const Fp6<Tw>& a, const Fp6<Tw>& b) {
    using F2 = typename Tw::F2;
    const F2 t0 = a.b0 * b.b0, t1 = a.b1 * b.b1, t2 = a.b2 * b.b2;
    Fp6<Tw> r;
    r.b0 = t0 + Tw::mul_xi((a.b1 + a.b2) * (b.b1 + b.b2) - t1 - t2);
    r.b1 = (a.b0 + a.b1) * (b.b0 + b.b1) - t0 - t1 + Tw::mul_xi(t2);
    r.b2 = (a.b0 + a.b2) * (b.b0 + b.b2) - t0 - t2 + t1;
    return r;
}
// a (b0 + b1 v), 5 Fp2 products
template <class Tw>
GG_HDN Fp6<Tw> mul_by_01(const Fp6<Tw>& a, const typename Tw::F2& b0, const typename Tw::F2& b1) {
    using F2 = typename Tw::F2;
    const F2 t0 = a.b0 * b0, t1 = a.b1 * b1;
    Fp6<Tw> r;
    r.b0 = t0 + Tw::mul_xi((a.b1 + a.b2) * b1 - t1);
    r.b1 = (a.b0 + a.b1) * (b0 + b1) - t0 - t1;
    r.b2 = (a.b0 + a.b2) * b0 - t0 + t1;
    return r;
}
template <class Tw>
GG_HD Fp6<Tw> mul_by_fp2(const Fp6<Tw>& a, const typename Tw::F2& s) {
    return Fp6<Tw>{a.b0 * s, a.b1 * s, a.b2 * s};
}
template <class Tw>
GG_HDN Fp6<Tw> inverse(const Fp6<Tw>& a) {
    using F2 = typename Tw::F2;
    const F2 c0 = sqr(a.b0) - Tw::mul_xi(a.b1 * a.b2);
    const F2 c1 = Tw::mul_xi(sqr(a.b2)) - a.b0 * a.b1;
    const F2 c2 = sqr(a.b1) - a.b0 * a.b2;
    const F2 t = inverse(a.b0 * c0 + Tw::mul_xi(a.b2 * c1 + a.b1 * c2));
    return Fp6<Tw>{c0 * t, c1 * t, c2 * t};
}

// ---------------------------------------------------------------- Fp12
template <class Tw>
GG_HDN Fp12<Tw> operator*(const Fp12<Tw>& a, const Fp12<Tw>& b) {
    const Fp6<Tw> t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    Fp12<Tw> r;
    r.c1 = (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1;
    r.c0 = t0 + mul_v(t1);
    return r;
}
template <class Tw>
GG_HDN Fp12<Tw> sqr(const Fp12<Tw>& a) {
    const Fp6<Tw> ab = a.c0 * a.c1;
    Fp12<Tw> r;
    r.c0 = (a.c0 + a.c1) * (a.c0 + mul_v(a.c1)) - ab - mul_v(ab);
    r.c1 = ab + ab;
    return r;
}
template <class Tw>
GG_HD Fp12<Tw> conj(const Fp12<Tw>& a) {
    return Fp12<Tw>{a.c0, -a.c1};
}
// through the norm to Fp6 (and from there to Fp2 and Fp): one Fp inversion
template <class Tw>
GG_HDN Fp12<Tw> inverse(const Fp12<Tw>& a) {
    const Fp6<Tw> t = inverse(a.c0 * a.c0 - mul_v(a.c1 * a.c1));
    return Fp12<Tw>{a.c0 * t, -(a.c1 * t)};
}
// a^(p^K), K = 1, 2, 3: coefficient i of w^i is conjugated K times and
// multiplied by xi^(i (p^K - 1) / 6)
template <class Tw, int K>
GG_HDN Fp12<Tw> frobenius(const Fp12<Tw>& a) {
    using F2 = typename Tw::F2;
    auto cj = [](const F2& z) { return (K & 1) ? Tw::conj(z) : z; };
    Fp12<Tw> r;
    r.c0.b0 = cj(a.c0.b0);
    r.c1.b0 = cj(a.c1.b0) * Tw::template gamma<K, 1>();
    r.c0.b1 = cj(a.c0.b1) * Tw::template gamma<K, 2>();
    r.c1.b1 = cj(a.c1.b1) * Tw::template gamma<K, 3>();
    r.c0.b2 = cj(a.c0.b2) * Tw::template gamma<K, 4>();
    r.c1.b2 = cj(a.c1.b2) * Tw::template gamma<K, 5>();
    return r;
}
// Granger-Scott squaring in the cyclotomic subgroup (after the easy part):
// Fp12 as a cubic extension of Fp4 = Fp2[w^3], pairs (c0, c3), (c1, c4), (c2, c5)
template <class Tw>
GG_HDN Fp12<Tw> cyclotomic_sqr(const Fp12<Tw>& x) {
    using F2 = typename Tw::F2;
    const F2 &x0 = x.c0.b0, &x1 = x.c0.b1, &x2 = x.c0.b2, &x3 = x.c1.b0, &x4 = x.c1.b1, &x5 = x.c1.b2;
    const F2 s4 = sqr(x4), s0 = sqr(x0), s2 = sqr(x2), s3 = sqr(x3), s5 = sqr(x5), s1 = sqr(x1);
    const F2 t6 = sqr(x4 + x0) - s4 - s0;                  // 2 x0 x4
    const F2 t7 = sqr(x2 + x3) - s2 - s3;                  // 2 x2 x3
    const F2 t8 = Tw::mul_xi(sqr(x5 + x1) - s5 - s1);      // 2 x1 x5 xi
    const F2 a0 = Tw::mul_xi(s4) + s0;                     // x4^2 xi + x0^2
    const F2 a2 = Tw::mul_xi(s2) + s3;                     // x2^2 xi + x3^2
    const F2 a4 = Tw::mul_xi(s5) + s1;                     // x5^2 xi + x1^2
    Fp12<Tw> z;
    z.c0.b0 = dbl(a0 - x0) + a0;
    z.c0.b1 = dbl(a2 - x1) + a2;
    z.c0.b2 = dbl(a4 - x2) + a4;
    z.c1.b0 = dbl(t8 + x3) + t8;
    z.c1.b1 = dbl(t6 + x4) + t6;
    z.c1.b2 = dbl(t7 + x5) + t7;
    return z;
}
// a^x in the cyclotomic subgroup, bits of |x| from a compile-time constant;
// a negative x conjugates (the inverse in the cyclotomic subgroup)
template <class Tw>
GG_HDN Fp12<Tw> cyclotomic_exp_x(const Fp12<Tw>& a) {
    Fp12<Tw> r = a;
    for (int i = Tw::X_TOP - 1; i >= 0; i--) {  // bit X_TOP is the top bit of |x|
        r = cyclotomic_sqr(r);
        if ((Tw::X >> i) & 1) r = r * a;
    }
    if constexpr (Tw::X_NEGATIVE) r = conj(r);
    return r;
}

// ---------------------------------------------------------------- lines
template <class Tw>
struct Line {
    typename Tw::F2 a, b, c;  // D-twist: a yp + b xp w + c w^3; M-twist: c + b xp w^2 + a yp w^3
};
// D-twist: f (l0 + l1 w + l2 w^3), l0 at C0.B0, l1 at C1.B0, l2 at C1.B1: 13 Fp2 products.
// M-twist: f ((c + l1 v) + (l0 v) w), c at C0.B0, l1 at C0.B1, l0 at C1.B1: 5 + 3 + 5 = 13.
template <class Tw>
GG_HDN void mul_by_line(Fp12<Tw>& f, const Line<Tw>& l, const Affine<typename Tw::F>& p) {
    using F2 = typename Tw::F2;
    const F2 l0 = Tw::scale(l.a, p.y), l1 = Tw::scale(l.b, p.x);
    if constexpr (Tw::M_TWIST) {
        const Fp6<Tw> t0 = mul_by_01(f.c0, l.c, l1);
        const Fp6<Tw> t1 = mul_v(mul_by_fp2(f.c1, l0));
        const Fp6<Tw> s = mul_by_01(f.c0 + f.c1, l.c, l0 + l1);
        f.c1 = s - t0 - t1;
        f.c0 = t0 + mul_v(t1);
    } else {
        const Fp6<Tw> t0 = mul_by_fp2(f.c0, l0);
        const Fp6<Tw> t1 = mul_by_01(f.c1, l1, l.c);
        const Fp6<Tw> s = mul_by_01(f.c0 + f.c1, l0 + l1, l.c);
        f.c1 = s - t0 - t1;
        f.c0 = t0 + mul_v(t1);
    }
}
// T <- 2T and the tangent's coefficients (T not infinity, Y != 0)
template <class Tw>
GG_HDN Line<Tw> line_double(Jac<typename Tw::F2>& t) {
    using F2 = typename Tw::F2;
    const F2 A = sqr(t.x), B = sqr(t.y), C = sqr(B), ZZ = sqr(t.z);
    const F2 D = dbl(sqr(t.x + B) - A - C);
    const F2 E = A + dbl(A);
    const F2 z3 = dbl(t.y * t.z);
    Line<Tw> l;
    l.a = z3 * ZZ;
    l.b = -(E * ZZ);
    l.c = E * t.x - dbl(B);
    const F2 x3 = sqr(E) - dbl(D);
    t.y = E * (D - x3) - dbl(dbl(dbl(C)));
    t.x = x3;
    t.z = z3;
    return l;
}
// T <- T + Q and the chord's coefficients (Q affine, T != +-Q)
template <class Tw>
GG_HDN Line<Tw> line_add(Jac<typename Tw::F2>& t, const Affine<typename Tw::F2>& q) {
    using F2 = typename Tw::F2;
    const F2 ZZ = sqr(t.z);
    const F2 H = q.x * ZZ - t.x;
    const F2 r = q.y * (t.z * ZZ) - t.y;
    const F2 HH = sqr(H), HHH = H * HH, V = t.x * HH;
    const F2 z3 = t.z * H;
    Line<Tw> l;
    l.a = z3;
    l.b = -r;
    l.c = r * q.x - z3 * q.y;
    const F2 x3 = sqr(r) - HHH - dbl(V);
    t.y = r * (V - x3) - t.y * HHH;
    t.x = x3;
    t.z = z3;
    return l;
}
// pi(Q) and -pi^2(Q) on the twist: the two extra lines of the optimal ate loop
template <class Tw>
GG_HD Affine<typename Tw::F2> g2_frob1(const Affine<typename Tw::F2>& q) {
    return Affine<typename Tw::F2>{Tw::conj(q.x) * Tw::template gamma<1, 2>(), Tw::conj(q.y) * Tw::template gamma<1, 3>()};
}
template <class Tw>
GG_HD Affine<typename Tw::F2> g2_frob2_neg(const Affine<typename Tw::F2>& q) {
    return Affine<typename Tw::F2>{q.x * Tw::template gamma<2, 2>(), -(q.y * Tw::template gamma<2, 3>())};
}

// number of lines of one G2 operand: LOOP_STEPS doublings, an addition per set
// bit of LOOP_LO, the two Frobenius lines where the loop has them
template <class Tw>
constexpr int line_count() {
    int n = Tw::LOOP_STEPS + (Tw::FROBENIUS_LINES ? 2 : 0);
    for (int i = 0; i < Tw::LOOP_STEPS; i++) n += (int)((Tw::LOOP_LO >> i) & 1);
    return n;
}

// One G2 operand of a product: either a point walked by the loop (tab == null)
// or the precomputed lines of a fixed point, read in the loop's order.
template <class Tw>
struct G2Src {
    const Line<Tw>* tab = nullptr;
    Affine<typename Tw::F2> q;
    Jac<typename Tw::F2> t;
    int pos = 0;
    bool skip = false;  // an operand at infinity: the pair contributes 1
};
template <class Tw>
GG_HD void src_init(G2Src<Tw>& s, const Affine<typename Tw::F2>& q, const Line<Tw>* tab, bool p_is_inf) {
    s.tab = tab;
    s.q = q;
    s.t = Jac<typename Tw::F2>{q.x, q.y, Tw::F2::one()};
    s.pos = 0;
    s.skip = p_is_inf || q.is_inf();
}
template <class Tw>
GG_HD Line<Tw> src_double(G2Src<Tw>& s) {
    if (s.tab) return s.tab[s.pos++];
    return line_double<Tw>(s.t);
}
template <class Tw>
GG_HD Line<Tw> src_add(G2Src<Tw>& s, const Affine<typename Tw::F2>& q) {
    if (s.tab) return s.tab[s.pos++];
    return line_add<Tw>(s.t, q);
}

// f <- f * prod_j Miller(p[j], s[j]) over K pairs: one squaring of the
// accumulator per loop bit for all K pairs
template <class Tw, int K>
GG_HDN void miller_loop(Fp12<Tw>& f, const Affine<typename Tw::F>* p, G2Src<Tw>* s) {
    Fp12<Tw> g = Fp12<Tw>::one();
    for (int i = Tw::LOOP_STEPS - 1; i >= 0; i--) {
        if (i != Tw::LOOP_STEPS - 1) g = sqr(g);
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!s[j].skip) {
                const Line<Tw> l = src_double(s[j]);
                mul_by_line(g, l, p[j]);
            }
        }
        if ((Tw::LOOP_LO >> i) & 1) {
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (!s[j].skip) {
                    const Line<Tw> l = src_add(s[j], s[j].q);
                    mul_by_line(g, l, p[j]);
                }
            }
        }
    }
    if constexpr (Tw::FROBENIUS_LINES) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (!s[j].skip) {
                const Line<Tw> l1 = src_add(s[j], g2_frob1<Tw>(s[j].q));
                mul_by_line(g, l1, p[j]);
                const Line<Tw> l2 = src_add(s[j], g2_frob2_neg<Tw>(s[j].q));
                mul_by_line(g, l2, p[j]);
            }
        }
    }
    if constexpr (Tw::X_NEGATIVE) g = conj(g);
    f = f * g;
}
// the lines of a fixed operand, in the order miller_loop reads them
template <class Tw>
GG_HDN void line_table(const Affine<typename Tw::F2>& q, Line<Tw>* out) {
    if (q.is_inf()) return;
    Jac<typename Tw::F2> t{q.x, q.y, Tw::F2::one()};
    int n = 0;
    for (int i = Tw::LOOP_STEPS - 1; i >= 0; i--) {
        out[n++] = line_double<Tw>(t);
        if ((Tw::LOOP_LO >> i) & 1) out[n++] = line_add<Tw>(t, q);
    }
    if constexpr (Tw::FROBENIUS_LINES) {
        out[n++] = line_add<Tw>(t, g2_frob1<Tw>(q));
        out[n++] = line_add<Tw>(t, g2_frob2_neg<Tw>(q));
    }
}

// the hard part of a BLS12 curve: f^((x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3), f in
// the cyclotomic subgroup (cyclotomic_exp_x carries the sign of x)
template <class Tw>
GG_HDN Fp12<Tw> final_exp_hard_bls12(const Fp12<Tw>& f) {
    using T = Fp12<Tw>;
    T a = cyclotomic_exp_x(f) * conj(f);               // x - 1
    a = cyclotomic_exp_x(a) * conj(a);                 // (x - 1)^2
    const T b = cyclotomic_exp_x(a) * frobenius<Tw, 1>(a);                               // (x + p)
    const T c = cyclotomic_exp_x(cyclotomic_exp_x(b)) * frobenius<Tw, 2>(b) * conj(b);   // (x^2 + p^2 - 1)
    return c * cyclotomic_sqr(f) * f;                  // + 3
}
// f^((p^12 - 1) / r * m); BN254: m = 2x(6x^2 + 3x + 1); BLS12: m = 3
template <class Tw>
GG_HDN Fp12<Tw> final_exp(const Fp12<Tw>& f0) {
    using T = Fp12<Tw>;
    T f = conj(f0) * inverse(f0);            // p^6 - 1
    f = frobenius<Tw, 2>(f) * f;             // p^2 + 1
    if constexpr (Tw::HARD_PART_BLS12) {
        return final_exp_hard_bls12(f);
    } else {
        const T fx = cyclotomic_exp_x(f);
        const T f2x = cyclotomic_sqr(fx);
        const T f6x = cyclotomic_sqr(f2x) * f2x;
        const T f6x2 = cyclotomic_exp_x(f6x);
        const T f12x3 = cyclotomic_exp_x(cyclotomic_sqr(f6x2));
        const T a = f12x3 * f6x2 * f6x;          // 12x^3 + 6x^2 + 6x
        const T b = a * conj(f2x);               // 12x^3 + 6x^2 + 4x
        T r = a * f6x2 * f;                      // lambda0 = 12x^3 + 12x^2 + 6x + 1
        r = r * frobenius<Tw, 1>(b);             // lambda1 = b
        r = r * frobenius<Tw, 2>(a);             // lambda2 = a
        r = r * frobenius<Tw, 3>(b * conj(f));   // lambda3 = b - 1
        return r;
    }
}

// the product of k pairings of one lane: chunks of at most 3 pairs share a squaring
template <class Tw>
GG_HDN Fp12<Tw> pairing_product(int k, const Affine<typename Tw::F>* g1, const Affine<typename Tw::F2>* g2) {
    Fp12<Tw> f = Fp12<Tw>::one();
    int j = 0;
    while (j < k) {
        const int c = k - j >= 3 ? 3 : k - j;
        Affine<typename Tw::F> p[3];
        G2Src<Tw> s[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            if (t < c) {
                p[t] = g1[j + t];
                src_init<Tw>(s[t], g2[j + t], nullptr, p[t].is_inf());
            }
        }
        if (c == 3) miller_loop<Tw, 3>(f, p, s);
        else if (c == 2) miller_loop<Tw, 2>(f, p, s);
        else miller_loop<Tw, 1>(f, p, s);
        j += c;
    }
    return final_exp(f);
}

// ---------------------------------------------------------------- point checks
// 0 good (the infinity included), 1 not on the curve, 2 not in the r-torsion
// k P for k = r by plain double-and-add, bits from the scalar field's modulus;
// FF is the coordinate field (Tw::F2 on the twist, Tw::F on the curve)
//
// Called<FF> is FF with its products as real calls.  With the 12-limb fields
// the inlined doubling and addition make one loop body of 70 k instructions
// (Fp2Bls), past the reach of a short branch; the compiler's long branches then
// took the return-address registers s[30:31] of this leaf function as their
// scratch pair, and its return jumped back into itself: the kernel never
// ended.  With the products called, the body is a few hundred instructions,
// every branch is short, and the function saves its return address as any
// caller does (Tw::CALLED_POINT_OPS; BN254 keeps the inlined body).
template <class FF>
GG_HDN FF mul_call(const FF& a, const FF& b) {
    return a * b;
}
template <class FF>
GG_HDN FF sqr_call(const FF& a) {
    return sqr(a);
}
template <class FF>
struct Called {
    FF v;
    static GG_HD Called zero() { return Called{FF::zero()}; }
    static GG_HD Called one() { return Called{FF::one()}; }
    GG_HD bool is_zero() const { return v.is_zero(); }
    GG_HD bool operator==(const Called& o) const { return v == o.v; }
};
template <class FF>
GG_HD Called<FF> operator+(const Called<FF>& a, const Called<FF>& b) {
    return Called<FF>{a.v + b.v};
}
template <class FF>
GG_HD Called<FF> operator-(const Called<FF>& a, const Called<FF>& b) {
    return Called<FF>{a.v - b.v};
}
template <class FF>
GG_HD Called<FF> operator-(const Called<FF>& a) {
    return Called<FF>{-a.v};
}
template <class FF>
GG_HD Called<FF> dbl(const Called<FF>& a) {
    return Called<FF>{a.v + a.v};
}
template <class FF>
GG_HD Called<FF> operator*(const Called<FF>& a, const Called<FF>& b) {
    return Called<FF>{mul_call(a.v, b.v)};
}
template <class FF>
GG_HD Called<FF> sqr(const Called<FF>& a) {
    return Called<FF>{sqr_call(a.v)};
}
// a^(p - 2) in FpBls with the products as calls (p - 2 differs from p in the lowest limb only)
inline GG_HDN FpBls inv_call(const FpBls& a) {
    const Called<FpBls> b{a};
    Called<FpBls> acc = Called<FpBls>::one();
#pragma unroll
    for (int w = FpBlsCfg::N - 1; w >= 0; w--) {
        const uint32_t word = w == 0 ? FpBlsCfg::P[0] - 2u : FpBlsCfg::P[w];
        for (int i = 31; i >= 0; i--) {
            acc = sqr(acc);
            if ((word >> i) & 1) acc = acc * b;
        }
    }
    return acc.v;
}
// 1 / a over Called<Fp2Bls>: the norm's inverse by inv_call (the batch normalisations of
// ecntt_g2.hip and groth16_mpc_setup.hip)
inline GG_HDN Called<Fp2Bls> inverse(const Called<Fp2Bls>& a) {
    using C = Called<FpBls>;
    const C a0{a.v.a0}, a1{a.v.a1};
    const C ni{inv_call((sqr(a0) + sqr(a1)).v)};
    return Called<Fp2Bls>{Fp2Bls{(a0 * ni).v, (-(a1 * ni)).v}};
}
template <class Tw, class FF>
GG_HDN bool times_r_is_inf(const Affine<FF>& q) {
    using C = typename std::conditional<Tw::CALLED_POINT_OPS, Called<FF>, FF>::type;
    Jac<C> base;
    if constexpr (Tw::CALLED_POINT_OPS) base = Jac<C>::from_affine(Affine<C>{C{q.x}, C{q.y}});
    else base = Jac<C>::from_affine(q);
    Jac<C> acc = Jac<C>::inf();
    for (int i = 255; i >= 0; i--) {
        const uint64_t word = i >= 192 ? Tw::R3 : i >= 128 ? Tw::R2 : i >= 64 ? Tw::R1 : Tw::R0;
        acc = jac_dbl(acc);
        if ((word >> (i & 63)) & 1) acc = jac_add(acc, base);
    }
    return acc.is_inf();
}
template <class Tw>
GG_HD int g2_check(const Affine<typename Tw::F2>& q) {
    if (q.is_inf()) return 0;
    if (!(sqr(q.y) == sqr(q.x) * q.x + Tw::b_twist())) return 1;
    return times_r_is_inf<Tw, typename Tw::F2>(q) ? 0 : 2;
}
template <class Tw>
GG_HD int g1_check(const Affine<typename Tw::F>& p) {
    if (p.is_inf()) return 0;
    if (!(sqr(p.y) == sqr(p.x) * p.x + Tw::b_g1())) return 1;
    if constexpr (Tw::G1_COFACTOR_ONE) return 0;
    else return times_r_is_inf<Tw, typename Tw::F>(p) ? 0 : 2;
}

// ---------------------------------------------------------------- endomorphism checks
// The same answers as g1_check / g2_check from one or two multiplications by
// |x| (64 bits, weight 6) instead of the 255-bit one by r (gnark-crypto's
// IsInSubGroup; Scott, "A note on group membership tests", 2021):
//   G1: [x^2] phi(P) + P = 0, phi(x, y) = (beta x, y) acting as x^2 - 1 on G1;
//   G2: psi(Q) = [x] Q, x < 0, so psi(Q) + [|x|] Q = 0.
// The point loops run over Called<FF> as times_r_is_inf does.
template <class Tw, class FF>
GG_HDN Jac<Called<FF>> mul_x_abs(const Jac<Called<FF>>& a) {
    Jac<Called<FF>> acc = a;
    for (int i = Tw::X_TOP - 1; i >= 0; i--) {
        acc = jac_dbl(acc);
        if ((Tw::X >> i) & 1) acc = jac_add(acc, a);
    }
    return acc;
}
template <class Tw>
GG_HDN bool g1_endo_is_member(const Affine<typename Tw::F>& p) {
    using C = Called<typename Tw::F>;
    Jac<C> a{C{p.x} * C{Tw::endo_beta()}, C{p.y}, C::one()};
    a = mul_x_abs<Tw, typename Tw::F>(a);
    a = mul_x_abs<Tw, typename Tw::F>(a);
    return jac_add(a, Jac<C>{C{p.x}, C{p.y}, C::one()}).is_inf();
}
template <class Tw>
GG_HDN bool g2_endo_is_member(const Affine<typename Tw::F2>& q) {
    using C = Called<typename Tw::F2>;
    const Jac<C> base{C{q.x}, C{q.y}, C::one()};
    const Jac<C> a = mul_x_abs<Tw, typename Tw::F2>(base);
    const Jac<C> psi{C{Tw::conj(q.x)} * C{Tw::template endo_psi<0>()}, C{Tw::conj(q.y)} * C{Tw::template endo_psi<1>()},
                     C::one()};
    return jac_add(a, psi).is_inf();
}
template <class Tw>
GG_HD int g1_check_endo(const Affine<typename Tw::F>& p) {
    if (p.is_inf()) return 0;
    if (!(sqr(p.y) == sqr(p.x) * p.x + Tw::b_g1())) return 1;
    return g1_endo_is_member<Tw>(p) ? 0 : 2;
}
template <class Tw>
GG_HD int g2_check_endo(const Affine<typename Tw::F2>& q) {
    if (q.is_inf()) return 0;
    if (!(sqr(q.y) == sqr(q.x) * q.x + Tw::b_twist())) return 1;
    return g2_endo_is_member<Tw>(q) ? 0 : 2;
}

}  // namespace pairing
}  // namespace gg
