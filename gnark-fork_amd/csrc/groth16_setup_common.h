// What the two makers of a gg_g16_setup share (groth16_setup.hip: from the toxic
// waste; groth16_mpc_setup.hip: from a powers-of-tau SRS): the handle, the
// uint32 scan, the transposed system (k_count / k_fill) and the numbering of an
// accumulation round's threads (pending / k_work).  See groth16_setup.hip for
// the scheme.  The kernels are static: each translation unit has its own copy.
#pragma once
#include "common.h"
#include "field.cuh"
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

namespace gg {
namespace g16s {

constexpr uint32_t ACC_BLOCK = 256;
// uint32 exclusive scan: 256 threads x 8 items per block
constexpr uint32_t USCAN_PER = 8;
constexpr uint32_t USCAN_BLK = 256 * USCAN_PER;

// zeroed before it is freed (toxic waste / discrete logs)
struct WipeBuf : DevBuf {
    WipeBuf() = default;
    explicit WipeBuf(size_t b) : DevBuf(b) {}
    void wipe() {
        if (p && bytes) {
            (void)hipMemsetAsync(p, 0, bytes, hipStreamPerThread);
            (void)hipStreamSynchronize(hipStreamPerThread);
        }
    }
    void wipe_release() {
        wipe();
        release();
    }
    ~WipeBuf() { wipe(); }
};

// ---------------------------------------------------------------- uint32 scan
// out[i] = sum of in[0..i) for i < m (in place allowed: a thread reads its own
// items before it writes them); bsum[b] = the total of block b
static __global__ void __launch_bounds__(256) k_uscan_block(const uint32_t* in, uint32_t* out, size_t m, uint32_t* bsum) {
    __shared__ uint32_t sh[256];
    const size_t base = (size_t)blockIdx.x * USCAN_BLK + (size_t)threadIdx.x * USCAN_PER;
    uint32_t v[USCAN_PER];
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < USCAN_PER; k++) {
        v[k] = base + k < m ? in[base + k] : 0u;
        s += v[k];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = sh[threadIdx.x] - s;  // exclusive prefix of this thread
#pragma unroll
    for (uint32_t k = 0; k < USCAN_PER; k++) {
        if (base + k < m) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 255 && bsum) bsum[blockIdx.x] = sh[255];
}
static __global__ void __launch_bounds__(256) k_uscan_add(uint32_t* out, size_t m, const uint32_t* boff) {
    const size_t base = (size_t)(blockIdx.x + 1) * USCAN_BLK + (size_t)threadIdx.x * USCAN_PER;
    const uint32_t c = boff[blockIdx.x + 1];
#pragma unroll
    for (uint32_t k = 0; k < USCAN_PER; k++)
        if (base + k < m) out[base + k] += c;
}
// exclusive scan of in[0..m) into out[0..m); scratch from `tmp` (grow-only list)
static void uscan(const uint32_t* in, uint32_t* out, size_t m, hipStream_t st, std::vector<std::unique_ptr<DevBuf>>& tmp) {
    if (!m) return;
    const size_t nblk = (m + USCAN_BLK - 1) / USCAN_BLK;
    uint32_t* bsum = nullptr;
    if (nblk > 1) {
        tmp.emplace_back(new DevBuf(nblk * 4));
        bsum = tmp.back()->as<uint32_t>();
    }
    hipLaunchKernelGGL(k_uscan_block, dim3((unsigned)nblk), dim3(256), 0, st, in, out, m, bsum);
    GG_HIP(hipGetLastError());
    if (nblk <= 1) return;
    uscan(bsum, bsum, nblk, st, tmp);
    hipLaunchKernelGGL(k_uscan_add, dim3((unsigned)(nblk - 1)), dim3(256), 0, st, out, m, (const uint32_t*)bsum);
    GG_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- transpose
// key = side * n_wires + wire; row = 3 * constraint + side
static __global__ void __launch_bounds__(256) k_count(const uint32_t* off, const uint32_t* wire, uint32_t nrows, uint32_t nw,
                                               uint32_t* cnt) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t side = r % 3u;
    for (uint32_t t = off[r]; t < off[r + 1]; t++) atomicAdd(cnt + (size_t)side * nw + wire[t], 1u);
}
static __global__ void __launch_bounds__(256) k_fill(const uint32_t* off, const uint32_t* wire, const uint32_t* cidx,
                                              uint32_t nrows, uint32_t nw, const uint32_t* list_off, uint32_t* cursor,
                                              uint2* ent) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t side = r % 3u, j = r / 3u;
    for (uint32_t t = off[r]; t < off[r + 1]; t++) {
        const size_t key = (size_t)side * nw + wire[t];
        const uint32_t pos = list_off[key] + atomicAdd(cursor + key, 1u);
        ent[pos] = make_uint2(j, cidx[t]);
    }
}

// ---------------------------------------------------------------- accumulate
// items still to add for key k after the previous round: the list length
// (first) or the partials it wrote (none when it wrote its final sum)
__device__ __forceinline__ uint32_t pending(const uint32_t* prev_off, uint32_t k, bool first) {
    const uint32_t d = prev_off[k + 1] - prev_off[k];
    return first ? d : (d > 1u ? d : 0u);
}
// work[k] = threads of this round for key k (k < nk), work[nk] = 0; *mx = max;
// CHUNK items per thread (scalars: ACC_CHUNK of groth16_setup.hip; points: ACC_CHUNK_PTS)
template <uint32_t CHUNK>
__global__ void __launch_bounds__(256) k_work(const uint32_t* prev_off, uint32_t nk, int first, uint32_t* work,
                                              uint32_t* mx) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nk) return;
    uint32_t w = 0;
    if (k < nk) w = (pending(prev_off, k, first != 0) + CHUNK - 1) / CHUNK;
    work[k] = w;
    if (w > 1u) atomicMax(mx, w);
}

// The rounds of one accumulation over the keys [0, nk) whose lists list_off
// delimits: round r cuts what every key still has to add into chunks of CHUNK
// items, numbers the chunks (k_work, scan) and calls
//   launch(first, prev_off, thr_off, nthr, psrc, pdst)
// for one kernel of nthr threads: thread i adds chunk i - thr_off[k] of its key k
// and writes the key's final sum, or partial i into pdst (item_bytes each), which
// the next round reads as psrc under thr_off.  Partials are wiped before they are
// freed.
struct AccStats {
    size_t launches = 0;
    double kernel_ms = 0, threads = 0;
};
template <uint32_t CHUNK, class Launch>
static void acc_rounds(const uint32_t* list_off, size_t nk, size_t item_bytes, hipStream_t st,
                       std::vector<std::unique_ptr<DevBuf>>& tmp, AccStats& stats, Launch launch) {
    static_assert(CHUNK >= 16, "the round limit below assumes chunks of at least 16 items");
    struct Ev {  // destroyed on the error paths too
        hipEvent_t e = nullptr;
        Ev() { GG_HIP(hipEventCreate(&e)); }
        ~Ev() { (void)hipEventDestroy(e); }
    } ev0, ev1;
    auto rd32 = [&](const uint32_t* p) {
        uint32_t v = 0;
        GG_HIP(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
        return v;
    };
    DevBuf work((nk + 1) * 4), offA((nk + 1) * 4), offB((nk + 1) * 4), mx(16);
    WipeBuf pa, pb;
    const uint32_t* prev_off = list_off;
    uint32_t* thr_off = offA.as<uint32_t>();
    WipeBuf* psrc = &pa;
    WipeBuf* pdst = &pb;
    for (int round = 0;; round++) {
        GG_CHECK(round < 9, GG_ERR_INTERNAL, "accumulate: too many rounds");  // 16^8 = 2^32 entries
        GG_HIP(hipMemsetAsync(mx.p, 0, mx.bytes, st));
        hipLaunchKernelGGL(k_work<CHUNK>, dim3(grid_for(nk + 1, 256)), dim3(256), 0, st, prev_off, (uint32_t)nk,
                           round == 0 ? 1 : 0, work.as<uint32_t>(), mx.as<uint32_t>());
        GG_HIP(hipGetLastError());
        uscan(work.as<uint32_t>(), thr_off, nk + 1, st, tmp);
        const uint32_t nthr = rd32(thr_off + nk);
        const uint32_t maxw = rd32(mx.as<uint32_t>());
        if (nthr == 0) break;
        pdst->wipe_release();
        if (maxw > 1) pdst->alloc((size_t)nthr * item_bytes);
        GG_HIP(hipEventRecord(ev0.e, st));
        launch(round == 0, prev_off, (const uint32_t*)thr_off, nthr, (const void*)psrc->p, pdst->p);
        GG_HIP(hipGetLastError());
        GG_HIP(hipEventRecord(ev1.e, st));
        GG_WAIT_STREAM(st);
        float ms = 0;
        GG_HIP(hipEventElapsedTime(&ms, ev0.e, ev1.e));
        stats.kernel_ms += ms;
        stats.launches++;
        stats.threads += nthr;
        if (maxw <= 1) break;
        std::swap(psrc, pdst);
        prev_off = thr_off;
        thr_off = thr_off == offA.as<uint32_t>() ? offB.as<uint32_t>() : offA.as<uint32_t>();
    }
}

// ---------------------------------------------------------------- host
// the CSR of gg_r1cs_create_ex as both makers take it; returns the term count
inline size_t check_terms(size_t nw, size_t ncons, size_t ncoef, const uint32_t* off, const uint32_t* wire,
                          const uint32_t* cidx) {
    GG_CHECK(ncoef >= 1 && ncoef < 0xffffffffu, GG_ERR_INVALID_ARG, "empty coefficient table");
    const size_t nrows = 3 * ncons;
    GG_CHECK(off[0] == 0, GG_ERR_INVALID_ARG, "term_off[0] must be 0");
    for (size_t i = 0; i < nrows; i++)
        GG_CHECK(off[i] <= off[i + 1], GG_ERR_INVALID_ARG, "term_off not monotonic");
    const size_t nterms = off[nrows];
    GG_CHECK(nterms == 0 || (wire && cidx), GG_ERR_INVALID_ARG, "null term arrays");
    for (size_t t = 0; t < nterms; t++) {
        if (wire[t] >= nw)
            throw Error(GG_ERR_INVALID_ARG, "term " + std::to_string(t) + ": wire id " + std::to_string(wire[t]) +
                                                " out of range (n_wires " + std::to_string(nw) + ")");
        if (cidx[t] >= ncoef)
            throw Error(GG_ERR_INVALID_ARG, "term " + std::to_string(t) + ": coefficient id " +
                                                std::to_string(cidx[t]) + " out of range (n_coeffs " +
                                                std::to_string(ncoef) + ")");
    }
    GG_CHECK(3 * nw + nterms < 0xfffffff0u, GG_ERR_INVALID_ARG, "system too large (3 n_wires + terms >= 2^32)");
    return nterms;
}

template <class F>
static F pow2k(F x, int k) {
    for (int i = 0; i < k; i++) x = x * x;
    return x;
}

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        auto t1 = std::chrono::steady_clock::now();
        double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

}  // namespace g16s
}  // namespace gg

struct gg_g16_setup {
    int curve = 0, log_n = 0, device = 0;
    size_t nw = 0, nA = 0, nB = 0, nK = 0, nZ = 0, n_vk = 0, g1b = 0, g2b = 0;
    std::vector<size_t> n_ck, ck_base;
    std::vector<uint32_t> k_wire_index;
    size_t acc_chunk = 0, acc_launches = 0;
    bool from_srs = false;  // made by gg_groth16_setup_from_srs: gg_groth16_setup_contribute works on it
    // [0..9) as gg_groth16_setup_timings documents; [9..) the phases of the SRS path (GG_SETUP_MS_*)
    double ms[GG_SETUP_TIMING_SLOTS] = {};
    // points (public): G1 parts and G2 parts in HBM until read
    gg::DevBuf g1_A, g1_B, g1_K, g1_Z, vk_K, g1_abd /* alpha, beta, delta */, ck, ck_sigma;
    gg::DevBuf g2_B, g2_tail /* beta, delta, gamma, G, GRootSigmaNeg */;
    gg::DevBuf inf_a, inf_b;
};
