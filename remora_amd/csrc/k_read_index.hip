// k_read_index.hip — the read-id index of a POD5 dataset (io.Pod5Dataset): the 16-byte read ids of all files of a run as a
// sorted table on the device, searched by the names of a batch of BAM records.  Replaces the lookup inside
// pod5.DatasetReader (src/remora/io.py:427, src/remora/inference.py:481, src/remora/prepare_train_data.py:153,
// src/remora/parsers.py:2109, src/remora/io.py:2554): there a Python dict from id to (file, row), here 24 bytes per distinct id.
//
// A key is its 16 bytes read as two big-endian 64-bit words (hi = bytes 0-7, lo = bytes 8-15): the order of the table is the
// byte order of the ids, which is also the order of their canonical hexadecimal text.
//   build   split_keys      raw ids -> hi[], lo[], perm[i] = i
//           radix sort      (lo, perm), all 64 bits, stable
//           gather_hi       hi of the permuted entries
//           radix sort      (hi, perm), stable: entries are in (hi, lo) order, equal ids in the order they were given
//           mark_heads      1 where an entry's id differs from its predecessor's; exclusive scan -> its slot in the table
//           compact         the heads' ids and values into the table: of equal ids the one given first survives
//   lookup  one thread per name: the 8-4-4-4-12 text -> (hi, lo), binary search, the value or -1
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rmr_internal.h"
#include "rmr_stage.h"

using namespace rmr;

namespace {

constexpr unsigned RI_THREADS = 256;

__global__ __launch_bounds__(RI_THREADS) void split_keys_kernel(const uint8_t *__restrict__ keys, int64_t n, uint64_t *__restrict__ hi,
                                                                 uint64_t *__restrict__ lo, uint32_t *__restrict__ perm) {
    const int64_t i = (int64_t)blockIdx.x * RI_THREADS + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 k = reinterpret_cast<const ulonglong2 *>(keys)[i];  // (16-byte aligned: the start of a staged array)
    hi[i] = __builtin_bswap64(k.x);
    lo[i] = __builtin_bswap64(k.y);
    perm[i] = (uint32_t)i;
}

__global__ __launch_bounds__(RI_THREADS) void gather_hi_kernel(const uint64_t *__restrict__ hi, const uint32_t *__restrict__ perm, int64_t n,
                                                                uint64_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * RI_THREADS + threadIdx.x;
    if (j < n) out[j] = hi[perm[j]];
}

// hi_sorted[j], lo[perm[j]]: the id at place j of the sorted order
__global__ __launch_bounds__(RI_THREADS) void mark_heads_kernel(const uint64_t *__restrict__ hi_sorted, const uint64_t *__restrict__ lo,
                                                                 const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * RI_THREADS + threadIdx.x;
    if (j >= n) return;
    head[j] = j == 0 || hi_sorted[j] != hi_sorted[j - 1] || lo[perm[j]] != lo[perm[j - 1]];
}

__global__ __launch_bounds__(RI_THREADS) void compact_kernel(const uint64_t *__restrict__ hi_sorted, const uint64_t *__restrict__ lo,
                                                              const uint32_t *__restrict__ perm, const int64_t *__restrict__ values,
                                                              const uint32_t *__restrict__ head, const uint32_t *__restrict__ slot, int64_t n,
                                                              int64_t n_distinct, uint64_t *__restrict__ t_hi, uint64_t *__restrict__ t_lo,
                                                              int64_t *__restrict__ t_val) {
    const int64_t j = (int64_t)blockIdx.x * RI_THREADS + threadIdx.x;
    if (j >= n || !head[j]) return;
    const int64_t s = slot[j];
    if (s >= n_distinct) return;  // (the table was sized by the same scan: never true)
    const uint32_t p = perm[j];
    t_hi[s] = hi_sorted[j];
    t_lo[s] = lo[p];
    t_val[s] = values[p];
}

__device__ inline int hex_value(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    c |= 0x20;
    return (c >= 'a' && c <= 'f') ? c - 'a' + 10 : -1;
}

__global__ __launch_bounds__(RI_THREADS) void lookup_kernel(const uint64_t *__restrict__ t_hi, const uint64_t *__restrict__ t_lo,
                                                             const int64_t *__restrict__ t_val, int64_t n, const char *__restrict__ names,
                                                             const int64_t *__restrict__ name_off, int64_t base, int64_t m,
                                                             int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RI_THREADS + threadIdx.x;
    if (i >= m) return;
    const int64_t a = name_off[i], len = name_off[i + 1] - a;
    int64_t found = -1;
    if (len == 36 && n > 0) {
        const char *s = names + (a - base);  // the staged text starts at the first name's offset
        uint64_t w[2] = {0, 0};
        bool ok = true;
        int digits = 0;
#pragma unroll
        for (int k = 0; k < 36; ++k) {
            const int c = (unsigned char)s[k];
            if (k == 8 || k == 13 || k == 18 || k == 23) {
                ok = ok && c == '-';
            } else {
                const int v = hex_value(c);
                ok = ok && v >= 0;
                w[digits >> 4] = (w[digits >> 4] << 4) | (uint64_t)(v & 15);
                ++digits;
            }
        }
        if (ok) {
            int64_t lo = 0, hi = n;  // the first entry that is not below (w[0], w[1])
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                const uint64_t h = t_hi[mid];
                const bool below = h < w[0] || (h == w[0] && t_lo[mid] < w[1]);
                if (below) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && t_hi[lo] == w[0] && t_lo[lo] == w[1]) found = t_val[lo];
        }
    }
    out[i] = found;
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + RI_THREADS - 1) / RI_THREADS)); }

struct DevBlock {  // the temporaries of one build: one allocation, freed when the call returns
    void *p = nullptr;
    ~DevBlock() { if (p) (void)hipFree(p); }
};

}  // namespace

namespace rmr {

// rocPRIM's scratch for one sort or the scan of n entries, whichever is larger
static int sort_scratch_bytes(int64_t n, size_t *bytes) {
    size_t sort_b = 0, scan_b = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    RMR_HIP(rocprim::radix_sort_pairs(nullptr, sort_b, k, k, v, v, (size_t)n, 0, 64, nullptr));
    RMR_HIP(rocprim::exclusive_scan(nullptr, scan_b, v, v, 0u, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
    *bytes = (sort_b > scan_b ? sort_b : scan_b) + 256;
    return 0;
}

int read_index_build(rmr_engine *e, const uint8_t *keys, const int64_t *values, int64_t n, rmr_read_index *ix) {
    // one block of temporaries: raw ids, values, hi, lo, two (key, perm) pairs for the sorts, heads, slots, rocPRIM's scratch
    size_t scratch = 0;
    RMR_TRY(sort_scratch_bytes(n, &scratch));
    Stage st;  // (for its layout only: the block is not the engine's arena, which never shrinks - a run's build would stay resident)
    uint8_t *d_keys, *d_tmp;
    int64_t *d_val;
    uint64_t *d_hi, *d_lo, *d_ka, *d_kb;
    uint32_t *d_pa, *d_pb, *d_head, *d_slot;
    st.add(&d_keys, (size_t)n * 16).add(&d_val, n).add(&d_hi, n).add(&d_lo, n).add(&d_ka, n).add(&d_kb, n).add(&d_pa, n).add(&d_pb, n);
    st.add(&d_head, n).add(&d_slot, n).add(&d_tmp, scratch);
    DevBlock blk;
    if (hipMalloc(&blk.p, st.total) != hipSuccess) {
        (void)hipGetLastError();
        RMR_FAIL(RMR_ERR_NOMEM, "the read-id index of %lld reads needs %zu bytes of device memory to build and they could not be allocated",
                 (long long)n, st.total);
    }
    for (const Stage::Slot &s : st.slots) s.set(s.where, static_cast<char *>(blk.p) + s.off);
    H2D(d_keys, keys, (size_t)n * 16);
    H2D(d_val, values, (size_t)n * 8);
    uint32_t last[2] = {0, 0};
    {
        ProfScope ps(e, K_READ_INDEX_BUILD);
        hipLaunchKernelGGL(split_keys_kernel, grid_of(n), dim3(RI_THREADS), 0, e->stream, d_keys, n, d_hi, d_lo, d_pa);
        size_t tb = scratch;
        RMR_HIP(rocprim::radix_sort_pairs(d_tmp, tb, d_lo, d_ka, d_pa, d_pb, (size_t)n, 0, 64, e->stream));
        hipLaunchKernelGGL(gather_hi_kernel, grid_of(n), dim3(RI_THREADS), 0, e->stream, d_hi, d_pb, n, d_ka);
        tb = scratch;
        RMR_HIP(rocprim::radix_sort_pairs(d_tmp, tb, d_ka, d_kb, d_pb, d_pa, (size_t)n, 0, 64, e->stream));
        // d_kb: hi in table order, d_pa: the entry at each place
        hipLaunchKernelGGL(mark_heads_kernel, grid_of(n), dim3(RI_THREADS), 0, e->stream, d_kb, d_lo, d_pa, n, d_head);
        tb = scratch;
        RMR_HIP(rocprim::exclusive_scan(d_tmp, tb, d_head, d_slot, 0u, (size_t)n, rocprim::plus<uint32_t>(), e->stream));
        RMR_HIP(hipGetLastError());
    }
    D2H(&last[0], d_head + (n - 1), 4);
    D2H(&last[1], d_slot + (n - 1), 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    const int64_t nd = (int64_t)last[0] + (int64_t)last[1];
    if (nd < 1 || nd > n) RMR_FAIL(RMR_ERR_HIP, "read-id index: %lld distinct ids out of %lld", (long long)nd, (long long)n);
    const size_t table_b = (size_t)nd * 24;
    if (hipMalloc(&ix->mem, table_b) != hipSuccess) {
        (void)hipGetLastError();
        ix->mem = nullptr;
        RMR_FAIL(RMR_ERR_NOMEM, "the read-id index of %lld distinct reads needs %zu bytes of device memory and they could not be allocated",
                 (long long)nd, table_b);
    }
    ix->hi = static_cast<uint64_t *>(ix->mem);
    ix->lo = ix->hi + nd;
    ix->val = reinterpret_cast<int64_t *>(ix->lo + nd);
    ix->n = nd;
    {
        ProfScope ps(e, K_READ_INDEX_BUILD);
        hipLaunchKernelGGL(compact_kernel, grid_of(n), dim3(RI_THREADS), 0, e->stream, d_kb, d_lo, d_pa, d_val, d_head, d_slot, n, nd, ix->hi,
                           ix->lo, ix->val);
        RMR_HIP(hipGetLastError());
    }
    RMR_HIP(hipStreamSynchronize(e->stream));  // the temporaries go when this returns
    return 0;
}

int launch_read_index_lookup(rmr_engine *e, const rmr_read_index *ix, const char *names, const int64_t *name_off, int64_t base, int64_t m,
                             int64_t *out) {
    if (m <= 0) return 0;
    ProfScope ps(e, K_READ_INDEX_LOOKUP);
    hipLaunchKernelGGL(lookup_kernel, grid_of(m), dim3(RI_THREADS), 0, e->stream, ix->hi, ix->lo, ix->val, ix->n, names, name_off, base, m, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
