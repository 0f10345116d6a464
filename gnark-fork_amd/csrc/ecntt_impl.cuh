// The EC-NTT's kernels and driver (see ecntt.hip), templated on the coordinate
// field F and the scalar field: ecntt.hip instantiates them over G1 (Fp, FpBls),
// ecntt_g2.hip over G2 (Fp2, Called<Fp2Bls>).
#pragma once
#include "ecntt.h"
#include "field.cuh"
#include "curve.cuh"
#include "comb.h"
#include "plonk_ops.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace gg {
namespace ecntt {

using comb::cld;
using comb::cst;

constexpr int BLOCK = 128;
// A stage with at least a wave of blocks (s >= 6), or with less than a wave of
// butterflies per block, indexes its threads butterfly-major: the lanes of a
// wave then share one twiddle, so they add at the same digits (no divergence
// in the double-and-add) and the skipped t = 1 butterflies fill whole waves
// instead of one lane in each.  Only the first six stages of a large transform
// run block-major, with a different twiddle in every lane: there a wave pays
// the addition at nearly every digit of the non-adjacent form (a wave adds
// wherever any lane has a digit); signed 4-bit windows add at the same places
// in every lane.  Measured (profiles/r09_plonk_setup.md), the windows win in
// the stages with a shared twiddle too (65 additions against 85), so every
// multiplying stage uses them; GG_ECNTT_MUL=naf keeps the table-free form for
// comparison.  The table of a window stage holds 8 points per thread in HBM:
// a stage runs in chunks of at most WINDOW_CHUNK threads that reuse one table.
constexpr uint32_t WAVE = 64;
constexpr uint32_t WINDOW_CHUNK = 1u << 20;
enum { MUL_WINDOW = 0, MUL_NAF = 1 };  // GG_ECNTT_MUL=naf (A/B: tools/bench_plonk_setup.py)

template <class SC>
__global__ void __launch_bounds__(256) k_fill_geo(Fe<SC>* x, size_t n, Fe<SC> first, Fe<SC> ratio) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cst(x + i, i ? ratio : first);
}

template <class F>
__global__ void __launch_bounds__(256) k_load(const Affine<F>* in, Xyzz<F>* x, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cst(x + i, Xyzz<F>::from_affine(cld(in + i)));
}

// acc = t * (*pp), t canonical; *pp is read again for every addition
template <class F, class SC>
__device__ __forceinline__ Xyzz<F> scalar_mul(const Xyzz<F>* pp, const Fe<SC>& t) {
    uint32_t k[9], h[9];  // t and 3 t (t < 2^255: 3 t < 2^257)
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        k[i] = t.v[i];
        c += 3ull * t.v[i];
        h[i] = (uint32_t)c;
        c >>= 32;
    }
    k[8] = 0;
    h[8] = (uint32_t)c;
    Xyzz<F> acc = Xyzz<F>::inf();
    for (int i = 256; i >= 1; i--) {
        acc = xyzz_dbl(acc);
        const uint32_t hb = (h[i >> 5] >> (i & 31)) & 1u, kb = (k[i >> 5] >> (i & 31)) & 1u;
        if (hb != kb) {
            Xyzz<F> q = cld(pp);
            if (kb) q.y = -q.y;
            xyzz_add_inplace(acc, q);
        }
    }
    return acc;
}

// t * (*pp) by signed 4-bit windows, t canonical: t + 0x88..8 has the nibbles
// d_i + 8 with d_i in [-8, 7] and sum d_i 16^i = t (i < 64; nibble 64 is the
// carry, 0 or 1, taken as it is).  tab[e * stride] receives (e + 1) P, e < 8
// (a doubling and 6 additions); then 64 x 4 doublings and at most 65 additions.
template <class F, class SC>
__device__ __forceinline__ Xyzz<F> scalar_mul_window(const Xyzz<F>* pp, const Fe<SC>& t, Xyzz<F>* tab,
                                                     size_t stride) {
    uint32_t k[9];
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = __builtin_addc(t.v[i], 0x88888888u, c, &c);
    k[8] = c;
    {  // two points live at a time, as in the loop below
        const Xyzz<F> p1 = cld(pp);
        Xyzz<F> q = p1;
        cst(tab, q);
#pragma unroll 1
        for (int e = 1; e < 8; e++) {
            if (e == 1) q = xyzz_dbl(q);
            else xyzz_add_inplace(q, p1);
            cst(tab + e * stride, q);
        }
    }
    Xyzz<F> acc = Xyzz<F>::inf();
    for (int i = 64; i >= 0; i--) {
        if (i != 64) {
            acc = xyzz_dbl(acc);
            acc = xyzz_dbl(acc);
            acc = xyzz_dbl(acc);
            acc = xyzz_dbl(acc);
        }
        const int nib = (int)((k[i >> 3] >> ((i & 7) * 4)) & 15u);
        const int d = i == 64 ? nib : nib - 8;
        if (d != 0) {
            Xyzz<F> q = cld(tab + (size_t)((d < 0 ? -d : d) - 1) * stride);
            if (d < 0) q.y = -q.y;
            xyzz_add_inplace(acc, q);
        }
    }
    return acc;
}

// stage s of the DIF over x[0..n): half = n >> (s + 1) butterflies per block;
// threads t0 .. t0 + cnt of the stage.  WIN: multiply by windows (tab: 8 * cnt
// points), else by the non-adjacent form (two kernels: the window one needs
// more registers)
template <class F, class SC, bool WIN>
__global__ void __launch_bounds__(BLOCK) k_stage(Xyzz<F>* x, const Fe<SC>* tw, Fe<SC> n_inv, uint32_t log_n,
                                                 uint32_t s, uint32_t t0, uint32_t cnt, Xyzz<F>* tab) {
    const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = t0 + local;
    const uint32_t log_half = log_n - 1u - s;
    if (local >= cnt || t >= (1u << (log_n - 1u))) return;
    const uint32_t half = 1u << log_half;
    uint32_t j, blk;
    if ((1u << s) < WAVE && half >= WAVE) {
        j = t & (half - 1u);
        blk = t >> log_half;
    } else {
        blk = t & ((1u << s) - 1u);
        j = t >> s;
    }
    Xyzz<F>* plo = x + (((size_t)blk << (log_half + 1u)) + j);
    Xyzz<F>* phi = plo + half;
    const Xyzz<F> a = cld(plo);
    Xyzz<F> b = cld(phi);
    {
        Xyzz<F> sum = a;
        xyzz_add_inplace(sum, b);
        cst(plo, sum);
    }
    b.y = -b.y;
    xyzz_add_inplace(b, a);  // a - b
    cst(phi, b);
    Fe<SC> w = cld(tw + ((size_t)j << s));
    if (blk == 0) w = w * n_inv;
    if (w == Fe<SC>::one() || b.is_inf()) return;
    if (WIN) cst(phi, scalar_mul_window<F, SC>(phi, from_mont(w), tab + local, cnt));
    else cst(phi, scalar_mul<F, SC>(phi, from_mont(w)));
}

// x[0] *= 1/n (the one output that never took a `hi` turn)
template <class F, class SC>
__global__ void __launch_bounds__(64) k_scale_first(Xyzz<F>* x, Fe<SC> n_inv) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (cld(x).is_inf()) return;
    cst(x, scalar_mul<F, SC>(x, from_mont(n_inv)));
}

// comb.h's k_comb_normalize with the output bit-reversed: thread t owns elements
// t, t + T, ...; one inversion per thread
template <class F>
__global__ void __launch_bounds__(256) k_normalize_brev(const Xyzz<F>* cur, size_t n, size_t T, uint32_t log_n,
                                                        F* prefix, Affine<F>* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || t >= n) return;
    F acc = F::one();
    for (size_t i = t; i < n; i += T) {
        cst(prefix + i, acc);
        const Xyzz<F> p = cld(cur + i);
        if (!p.is_inf()) acc = acc * p.zzz;
    }
    F inv = inverse(acc);
    const size_t last = t + ((n - 1 - t) / T) * T;
    for (size_t i = last;; i -= T) {
        const Xyzz<F> p = cld(cur + i);
        const size_t o = __brev((uint32_t)i) >> (32u - log_n);
        if (p.is_inf()) {
            cst(out + o, Affine<F>::inf());
        } else {
            const F izzz = inv * cld(prefix + i);
            inv = inv * p.zzz;
            const F izz = sqr(izzz) * sqr(p.zz);
            cst(out + o, Affine<F>{p.x * izz, p.y * izzz});
        }
        if (i < T) break;
    }
}

template <class SC>
static Fe<SC> pow2k(Fe<SC> x, int k) {
    for (int i = 0; i < k; i++) x = x * x;
    return x;
}

inline int mul_mode() {
    const char* e = getenv("GG_ECNTT_MUL");
    return e && !strcmp(e, "naf") ? MUL_NAF : MUL_WINDOW;
}

// threads per launch of a window stage (GG_ECNTT_WINDOW_CHUNK: tests cross the
// chunk boundary at a small size with it)
inline size_t window_chunk() {
    const char* e = getenv("GG_ECNTT_WINDOW_CHUNK");
    const long v = e ? atol(e) : 0;
    if (v <= 0) return WINDOW_CHUNK;
    return std::min<size_t>(WINDOW_CHUNK, ((size_t)v + BLOCK - 1) / BLOCK * BLOCK);
}

struct Ev {
    hipEvent_t e = nullptr;
    Ev() { GG_HIP(hipEventCreate(&e)); }
    ~Ev() { (void)hipEventDestroy(e); }
};

template <class F, class SC>
void run(int log_n, const void* omega_mont, const Affine<F>* in, Affine<F>* out, hipStream_t st, double* ms) {
    using S = Fe<SC>;
    const size_t n = (size_t)1 << log_n, nh = n / 2;
    S omega;
    memcpy(&omega, omega_mont, sizeof(omega));
    const S w = inverse(omega);
    S nf = S::zero();
    nf.v[0] = (uint32_t)n;  // n <= 2^27
    const S n_inv = inverse(to_mont(nf));

    // w^j, j < n / 2 (Montgomery; a stage reads every 2^s-th)
    DevBuf tw(nh * sizeof(S));
    {
        Arena ar;
        ar.reserve(plk::scan_arena_bytes(nh) + 4096);
        hipLaunchKernelGGL(k_fill_geo<SC>, dim3(grid_for(nh, 256)), dim3(256), 0, st, tw.as<S>(), nh, S::one(), w);
        GG_HIP(hipGetLastError());
        if (nh > 1) plk::scan_prod(tw.as<S>(), nh, st, ar);
        GG_WAIT_STREAM(st);  // the arena goes away here
    }
    DevBuf x(n * sizeof(Xyzz<F>));
    Ev e0, e1, e2;
    GG_HIP(hipEventRecord(e0.e, st));
    hipLaunchKernelGGL(k_load<F>, dim3(grid_for(n, 256)), dim3(256), 0, st, in, x.as<Xyzz<F>>(), n);
    GG_HIP(hipGetLastError());
    const int mode = mul_mode();
    DevBuf tab;
    for (int s = 0; s < log_n; s++) {
        const bool window = mode == MUL_WINDOW && s + 1 < log_n;  // the last stage multiplies block 0 only
        const size_t chunk = window ? std::min<size_t>(nh, window_chunk()) : nh;
        if (window) tab.reserve(8 * chunk * sizeof(Xyzz<F>));
        for (size_t t0 = 0; t0 < nh; t0 += chunk) {
            if (window)
                hipLaunchKernelGGL((k_stage<F, SC, true>), dim3(grid_for(chunk, BLOCK)), dim3(BLOCK), 0, st,
                                   x.as<Xyzz<F>>(), (const S*)tw.p, n_inv, (uint32_t)log_n, (uint32_t)s, (uint32_t)t0,
                                   (uint32_t)chunk, tab.as<Xyzz<F>>());
            else
                hipLaunchKernelGGL((k_stage<F, SC, false>), dim3(grid_for(chunk, BLOCK)), dim3(BLOCK), 0, st,
                                   x.as<Xyzz<F>>(), (const S*)tw.p, n_inv, (uint32_t)log_n, (uint32_t)s, (uint32_t)t0,
                                   (uint32_t)chunk, (Xyzz<F>*)nullptr);
            GG_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL((k_scale_first<F, SC>), dim3(1), dim3(64), 0, st, x.as<Xyzz<F>>(), n_inv);
    GG_HIP(hipGetLastError());
    GG_HIP(hipEventRecord(e1.e, st));
    DevBuf prefix(n * sizeof(F));
    const size_t T = std::min<size_t>(n, std::max<size_t>(16384, n / 64));
    hipLaunchKernelGGL(k_normalize_brev<F>, dim3(grid_for(T, 256)), dim3(256), 0, st, (const Xyzz<F>*)x.p, n, T,
                       (uint32_t)log_n, prefix.as<F>(), out);
    GG_HIP(hipGetLastError());
    GG_HIP(hipEventRecord(e2.e, st));
    GG_WAIT_STREAM(st);
    if (ms) {
        float a = 0, b = 0;
        GG_HIP(hipEventElapsedTime(&a, e0.e, e1.e));
        GG_HIP(hipEventElapsedTime(&b, e1.e, e2.e));
        ms[0] = a;
        ms[1] = b;
    }
}

}  // namespace ecntt
}  // namespace gg
