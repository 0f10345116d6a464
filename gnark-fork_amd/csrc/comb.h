// The 8-bit fixed-base comb of batch.hip for a caller with many scalar vectors
// for one base (Groth16 Setup: every G1 part is a multiple of the G1 generator):
// the table is built once per generator and device-resident scalars are
// multiplied into device-resident outputs.  Header only (the EC-NTT and the
// setup from an SRS use its loads, stores and batch normalisation too);
// batch.hip keeps its own copy of the same method
// (gg_batch_scalar_mul: table, multiply and copy in one call) untouched.
//   T[w][j] = j * 2^(8w) * B (32 x 256 affine points, built on the host);
//   a scalar is 32 table lookups + 31 mixed XYZZ additions; the XYZZ results
//   are batch-normalised to affine on the device (k = 0 -> all-zero affine).
#pragma once
#include "common.h"
#include "curve.cuh"
#include <algorithm>
#include <vector>

namespace gg {
namespace comb {

template <class T>
__device__ __forceinline__ T cld(const T* p) {
    static_assert(sizeof(T) % 16 == 0, "16B multiple");
    T r;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 16); i++) d[i] = s[i];
    return r;
}
template <class T>
__device__ __forceinline__ void cst(T* p, const T& v) {
    uint4* d = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 16); i++) d[i] = s[i];
}

template <class F, class SC>
__global__ void __launch_bounds__(256) k_comb_mul(const Affine<F>* table, const Fe<SC>* scalars, size_t n,
                                                  Xyzz<F>* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<SC> k = from_mont(cld(scalars + i));
    Xyzz<F> acc = Xyzz<F>::inf();
    for (int w = 0; w < 32; w++) {
        uint32_t j = (k.v[w >> 2] >> ((w & 3) * 8)) & 0xffu;
        if (j) acc = xyzz_madd(acc, cld(table + w * 256 + j));
    }
    cst(out + i, acc);
}

// thread t owns elements t, t + T, ...: one inversion per thread
template <class F>
__global__ void __launch_bounds__(256) k_comb_normalize(const Xyzz<F>* cur, size_t n, size_t T, F* prefix,
                                                        Affine<F>* out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || t >= n) return;
    F acc = F::one();
    for (size_t i = t; i < n; i += T) {
        cst(prefix + i, acc);
        Xyzz<F> p = cld(cur + i);
        if (!p.is_inf()) acc = acc * p.zzz;
    }
    F inv = inverse(acc);
    size_t last = t + ((n - 1 - t) / T) * T;
    for (size_t i = last;; i -= T) {
        Xyzz<F> p = cld(cur + i);
        if (p.is_inf()) {
            cst(out + i, Affine<F>::inf());
        } else {
            F izzz = inv * cld(prefix + i);
            inv = inv * p.zzz;
            F izz = sqr(izzz) * sqr(p.zz);
            cst(out + i, Affine<F>{p.x * izz, p.y * izzz});
        }
        if (i < T) break;
    }
}

template <class F>
struct CombTable {
    DevBuf tab;
    // host build (Montgomery batch inversion of the Z coordinates), upload on st
    void build(const Affine<F>& base, hipStream_t st) {
        std::vector<Jac<F>> J(32 * 256);
        Jac<F> bw = Jac<F>::from_affine(base);
        for (int w = 0; w < 32; w++) {
            J[w * 256] = Jac<F>::inf();
            for (int j = 1; j < 256; j++) J[w * 256 + j] = jac_add(J[w * 256 + j - 1], bw);
            for (int s = 0; s < 8; s++) bw = jac_dbl(bw);
        }
        std::vector<F> pre(J.size());
        F acc = F::one();
        for (size_t i = 0; i < J.size(); i++) {
            pre[i] = acc;
            if (!J[i].is_inf()) acc = acc * J[i].z;
        }
        F inv = inverse(acc);
        std::vector<Affine<F>> T(J.size());
        for (size_t i = J.size(); i-- > 0;) {
            if (J[i].is_inf()) {
                T[i] = Affine<F>::inf();
                continue;
            }
            F zi = inv * pre[i];
            inv = inv * J[i].z;
            F zi2 = sqr(zi);
            T[i] = Affine<F>{J[i].x * zi2, J[i].y * zi2 * zi};
        }
        tab.alloc(T.size() * sizeof(Affine<F>));
        GG_HIP(hipMemcpyAsync(tab.p, T.data(), tab.bytes, hipMemcpyHostToDevice, st));
        GG_WAIT_STREAM(st);  // the host table goes away with this call
    }
};

// scratch (grow-only): the XYZZ sums and the normalisation prefixes
struct CombScratch {
    DevBuf cur, prefix;
};

// out_dev[i] = scalars_dev[i] * base (affine, infinity for 0), n > 0, enqueued on st
template <class F, class SC>
void comb_mul(const CombTable<F>& t, const Fe<SC>* scalars_dev, size_t n, Affine<F>* out_dev, CombScratch& scratch,
              hipStream_t st) {
    scratch.cur.reserve(n * sizeof(Xyzz<F>));
    scratch.prefix.reserve(n * sizeof(F));
    hipLaunchKernelGGL((k_comb_mul<F, SC>), dim3(grid_for(n, 256)), dim3(256), 0, st, (const Affine<F>*)t.tab.p,
                       scalars_dev, n, scratch.cur.as<Xyzz<F>>());
    GG_HIP(hipGetLastError());
    const size_t T = std::min<size_t>(n, std::max<size_t>(16384, n / 64));
    hipLaunchKernelGGL(k_comb_normalize<F>, dim3(grid_for(T, 256)), dim3(256), 0, st,
                       (const Xyzz<F>*)scratch.cur.p, n, T, scratch.prefix.as<F>(), out_dev);
    GG_HIP(hipGetLastError());
}

}  // namespace comb
}  // namespace gg
