// gnark-crypto's Fiat-Shamir transcript with the caller's hash (gg_hash_fn) or
// SHA-256, host only: shared by the PlonK prover (plonk_prover.hip) and the
// PlonK verifier (plonk_verify.hip), which must derive the same challenges.
#pragma once
#include "common.h"
#include "sha256.h"
#include <initializer_list>
#include <string>
#include <vector>

namespace gg {
namespace fs {

// canonical little-endian u32 limbs -> big-endian bytes
template <int N>
inline void be_bytes(const uint32_t* v, uint8_t* out) {
    for (int i = 0; i < N; i++) {
        const uint32_t w = v[N - 1 - i];
        out[4 * i] = (uint8_t)(w >> 24);
        out[4 * i + 1] = (uint8_t)(w >> 16);
        out[4 * i + 2] = (uint8_t)(w >> 8);
        out[4 * i + 3] = (uint8_t)w;
    }
}

struct Hasher {
    gg_hash_fn fn;
    void* ctx;
    std::vector<uint8_t> operator()(const std::vector<uint8_t>& msg) const {
        if (!fn) {
            std::vector<uint8_t> d(32);
            Sha256::hash(msg.data(), msg.size(), d.data());
            return d;
        }
        std::vector<uint8_t> d(128);
        size_t len = d.size();
        GG_CHECK(fn(ctx, msg.data(), msg.size(), d.data(), &len) == 0, GG_ERR_INVALID_ARG, "hash callback failed");
        GG_CHECK(len >= 1 && len <= 128, GG_ERR_INVALID_ARG, "hash callback: digest of 1..128 bytes");
        d.resize(len);
        return d;
    }
};

// fr.Element.SetBytes: big-endian integer mod r
template <class FrB>
inline FrB fr_set_bytes(const uint8_t* b, size_t n) {
    FrB acc = FrB::zero();
    FrB b256 = FrB::zero();
    b256.v[0] = 256;
    b256 = to_mont(b256);
    for (size_t i = 0; i < n; i++) {
        FrB d = FrB::zero();
        d.v[0] = b[i];
        acc = acc * b256 + to_mont(d);
    }
    return acc;
}

// gnark-crypto fiat-shamir Transcript: challenge i = H(name_i | value_(i-1) | bindings_i)
template <class FrB>
struct Transcript {
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> bound, value;
    Hasher h;
    Transcript(std::initializer_list<const char*> ns, Hasher hh) : h(hh) {
        for (const char* s : ns) names.emplace_back(s);
        bound.resize(names.size());
        value.resize(names.size());
    }
    size_t idx(const char* n) const {
        for (size_t i = 0; i < names.size(); i++)
            if (names[i] == n) return i;
        throw Error(GG_ERR_INTERNAL, "unknown challenge");
    }
    void bind(const char* n, const uint8_t* b, size_t len) {
        auto& v = bound[idx(n)];
        v.insert(v.end(), b, b + len);
    }
    FrB compute(const char* n) {
        const size_t i = idx(n);
        std::vector<uint8_t> msg(names[i].begin(), names[i].end());
        if (i) msg.insert(msg.end(), value[i - 1].begin(), value[i - 1].end());
        msg.insert(msg.end(), bound[i].begin(), bound[i].end());
        value[i] = h(msg);
        return fr_set_bytes<FrB>(value[i].data(), value[i].size());
    }
};

}  // namespace fs
}  // namespace gg
