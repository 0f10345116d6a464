// Host plumbing shared by the pairing translation units (pairing.hip,
// pairing_bls.hip) and the verifiers built on them: a private stream,
// host-or-device operands and results, the argument checks of the pairing entry
// points, the launch of a pairing product, of a point check and of one step of
// a verifier.
#pragma once
#include "common.h"
#include <string>
#include <vector>

namespace gg {
namespace pairing {

struct Stream {
    hipStream_t s = nullptr;
    Stream() { GG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};
// a device view of `bytes` at p: p itself when it is device memory, else an upload into buf
static inline const void* to_device(const void* p, size_t bytes, DevBuf& buf, hipStream_t st) {
    if (!bytes || is_device_ptr(p)) return p;
    buf.reserve(bytes);
    GG_HIP(hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, st));
    return buf.p;
}
// host copy of `bytes` at p (p itself when it is host memory)
static inline const uint8_t* to_host(const void* p, size_t bytes, std::vector<uint8_t>& buf) {
    if (!bytes || !is_device_ptr(p)) return (const uint8_t*)p;
    buf.resize(bytes);
    GG_HIP(hipMemcpy(buf.data(), p, bytes, hipMemcpyDeviceToHost));
    return buf.data();
}
// results: written through when out is device memory, else copied back from a
// device buffer (its own, or one the caller keeps across calls)
struct OutBuf {
    void* host = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
    DevBuf own;
    void init(void* out, size_t b) { init(out, b, own); }
    void init(void* out, size_t b, DevBuf& buf) {
        bytes = b;
        if (is_device_ptr(out)) {
            dev = out;
        } else {
            host = out;
            buf.reserve(b);
            dev = buf.p;
        }
    }
    void finish(hipStream_t st) {
        if (host) GG_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
    }
};

static inline void check_pairing_args(size_t n, int k, const void* g1, const void* g2, const void* out,
                                      const char* out_name) {
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(k > 0, GG_ERR_INVALID_ARG, "k must be > 0 (pairs per product)");
    GG_CHECK(n <= ((size_t)1 << 31) / (size_t)k, GG_ERR_INVALID_ARG, "n * k exceeds 2^31 pairs");
    GG_CHECK(g1, GG_ERR_INVALID_ARG, "null argument: g1");
    GG_CHECK(g2, GG_ERR_INVALID_ARG, "null argument: g2");
    GG_CHECK(out, GG_ERR_INVALID_ARG, std::string("null argument: ") + out_name);
}
static inline void check_points_args(size_t n, const void* pts, const char* name, const void* flags_out) {
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(pts, GG_ERR_INVALID_ARG, std::string("null argument: ") + name);
    GG_CHECK(flags_out, GG_ERR_INVALID_ARG, "null argument: flags_out");
}
// n products of k pairs on the device: the GT values, or whether each is one
template <class GT, class G1, class G2, class Kern>
static void run_pairing(Kern kern, size_t n, int k, const void* g1, const void* g2, void* gt_out, uint8_t* ok_out) {
    Stream st;
    DevBuf b1, b2;
    const size_t np = n * (size_t)k;
    const G1* d1 = (const G1*)to_device(g1, np * sizeof(G1), b1, st.s);
    const G2* d2 = (const G2*)to_device(g2, np * sizeof(G2), b2, st.s);
    OutBuf o;
    if (gt_out) o.init(gt_out, n * sizeof(GT));
    else o.init(ok_out, n);
    hipLaunchKernelGGL(kern, dim3(grid_for(n, 64)), dim3(64), 0, st.s, n, k, d1, d2, gt_out ? (GT*)o.dev : nullptr,
                       gt_out ? nullptr : (uint8_t*)o.dev);
    GG_HIP(hipGetLastError());
    o.finish(st.s);
}
template <class P, class Kern>
static void run_check(size_t n, const void* pts, uint8_t* flags, Kern kern, unsigned block) {
    Stream st;
    DevBuf b;
    const P* d = (const P*)to_device(pts, n * sizeof(P), b, st.s);
    OutBuf o;
    o.init(flags, n);
    hipLaunchKernelGGL(kern, dim3(grid_for(n, block)), dim3(block), 0, st.s, n, d, (uint8_t*)o.dev);
    GG_HIP(hipGetLastError());
    o.finish(st.s);
}
// One step of a verifier over `count` lanes: a kernel launch on st, or a loop on this thread.
template <class A>
static void run(bool dev, hipStream_t st, void (*kern)(A), void (*body)(const A&, size_t), const A& a, size_t count,
                unsigned block) {
    if (!count) return;
    if (dev) {
        hipLaunchKernelGGL(kern, dim3(grid_for(count, block)), dim3(block), 0, st, a);
        GG_HIP(hipGetLastError());
    } else {
        for (size_t i = 0; i < count; i++) body(a, i);
    }
}

}  // namespace pairing
}  // namespace gg
