// sort_probe.hip -- test probe (tests/test_gpu_sort.py): calls the radix sort of hx_sort.h exactly as hx_mapper.hip, the catalogue contexts
// and hx_nufft.hip do -- scratch pairs and `tmp` from DevBufs, the library's stream -- and copies the sorted pairs out.  No sort logic of its own; not part
// of the C ABI (include/hxsht.h).  Links against the in-tree libhxsht.so for the runtime (hx::rt, hx::ensure_ready, hx::fail, DevBuf).
#include "hx_common.h"
#include "hx_sort.h"

using namespace hx;

namespace {

template <class K>
int copy_out(const K *ks, const unsigned *vs, unsigned long long n, K *out_keys, unsigned *out_vals)
{
    hipStream_t st = rt().stream;
    if (n) {
        HX_HIP(hipMemcpyAsync(out_keys, ks, sizeof(K) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HX_HIP(hipMemcpyAsync(out_vals, vs, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
    HX_HIP(hipStreamSynchronize(st));
    return HX_OK;
}

// the input pair is overwritten by the sort: it is copied into a DevBuf pair first, as the callers' key kernels fill theirs
template <class K>
int sort_full(const K *keys, const unsigned *vals, unsigned long long n, int end_bit, K *out_keys, unsigned *out_vals)
{
    HX_TRY(ensure_ready());
    hipStream_t st = rt().stream;
    DevBuf k0, v0, k1, v1, tmp;
    const size_t m = (size_t)(n ? n : 1);
    HX_TRY(k0.alloc(sizeof(K) * m));
    HX_TRY(k1.alloc(sizeof(K) * m));
    HX_TRY(v0.alloc(sizeof(unsigned) * m));
    HX_TRY(v1.alloc(sizeof(unsigned) * m));
    if (n) {
        HX_HIP(hipMemcpyAsync(k0.p, keys, sizeof(K) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HX_HIP(hipMemcpyAsync(v0.p, vals, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
    K *ks = nullptr;
    unsigned *vs = nullptr;
    HX_TRY(rsort::radix_sort_pairs<K>(k0.as<K>(), v0.as<unsigned>(), k1.as<K>(), v1.as<unsigned>(), n, end_bit, tmp, st, &ks, &vs));
    return copy_out(ks, vs, n, out_keys, out_vals);
}

}  // namespace

extern "C" {

int hxprobe_sort_u32(const unsigned *keys, const unsigned *vals, unsigned long long n, int end_bit, unsigned *out_keys, unsigned *out_vals)
{
    return sort_full<unsigned>(keys, vals, n, end_bit, out_keys, out_vals);
}

int hxprobe_sort_i64(const long long *keys, const unsigned *vals, unsigned long long n, int end_bit, long long *out_keys, unsigned *out_vals)
{
    return sort_full<long long>(keys, vals, n, end_bit, out_keys, out_vals);
}

// the 64-bit keys are read in place (const in the sort); ka / kb share one buffer as in hx_map_values
int hxprobe_sort_narrow(const long long *keys64, const unsigned *vals, unsigned long long n, int end_bit, unsigned *out_keys32,
                        unsigned *out_vals)
{
    HX_TRY(ensure_ready());
    hipStream_t st = rt().stream;
    DevBuf kab, v0, v1, tmp;
    const size_t m = (size_t)(n ? n : 1);
    HX_TRY(kab.alloc(sizeof(unsigned) * 2 * m));
    HX_TRY(v0.alloc(sizeof(unsigned) * m));
    HX_TRY(v1.alloc(sizeof(unsigned) * m));
    if (n) HX_HIP(hipMemcpyAsync(v0.p, vals, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, st));
    unsigned *ks = nullptr, *vs = nullptr;
    HX_TRY(rsort::radix_sort_pairs_narrow(keys64, v0.as<unsigned>(), kab.as<unsigned>(), kab.as<unsigned>() + n, v1.as<unsigned>(), n, end_bit,
                                          tmp, st, &ks, &vs));
    return copy_out(ks, vs, n, out_keys32, out_vals);
}

}  // extern "C"
