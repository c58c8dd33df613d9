// rmr_stage.h — the layout of one call's arrays in the engine's staging arena (RMR_MEM_HOST calls, the scratch of the device
// ones).  Every staged array is named ONCE, with its element count, where its pointer is declared: add() records the slot,
// commit() sizes the arena to the sum of the slots and hands out the pointers.  No byte count of the arena is written anywhere
// else.  Everything down to the two copy macros at the end is plain C++ without HIP (tests/c/stage_layout.cpp runs it on the CPU
// against a fake engine), including the slots of a batch of reads and of its chunks, which that test lays out as well.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/remora_hip.h"
#include "rmr_pack.h"  // RMR_TRY

namespace rmr {

struct Stage {
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    struct Slot {  // set(where, address): assigns the T* at `where`
        void *where;
        void (*set)(void *where, char *at);
        size_t off, bytes;
    };
    std::vector<Slot> slots;
    size_t total = 0;  // every slot starts on a 256-byte boundary; a slot of no elements is legal and takes no room

    template <typename T>
    Stage &add(T **ptr, size_t count) {
        slots.push_back({ptr, [](void *w, char *at) { *static_cast<T **>(w) = reinterpret_cast<T *>(at); }, total, count * sizeof(T)});
        total += pad(count * sizeof(T));
        return *this;
    }
    // `Engine`: rmr_engine (ensure() grows the arena; pointers into it from before a commit are stale after one that grew it)
    template <class Engine>
    int commit(Engine *e) {
        RMR_TRY(e->ensure(e->staging, total));
        for (const Slot &s : slots) s.set(s.where, reinterpret_cast<char *>(e->staging.ptr) + s.off);
        return 0;
    }
};

// device-side copy of an rmr_reads whose arrays live on the host
struct DevReads {
    rmr_reads d{};
    int32_t *chunk_read = nullptr;
    int64_t n_chunks = 0, total_sig = 0, total_bases = 0;
};

// The arrays of the rmr_reads `r` (nr reads) that a RMR_MEM_HOST call uploads into the DevReads `o`, X(field, elements to
// copy); dacs goes in front where the call reads the raw signal.  Each is declared one element longer than is copied: the
// kernels' vector loads run past the end.
#define RMR_READ_ARRAYS(X)                                                                                               \
    X(sig_off, nr + 1) X(seq_to_sig, o->total_bases + nr) X(int_seq, o->total_bases) X(seq_off, nr + 1) X(shift, nr) \
    X(scale, nr) X(focus_bases, o->n_chunks) X(focus_off, nr + 1)

// slots of a batch of reads: the read index of every chunk and, for host arrays, a device copy of each
inline void declare_reads(Stage &st, const rmr_reads *r, int mem, bool need_dacs, int64_t total_sig, int64_t total_bases,
                          int64_t n_chunks, DevReads *o) {
    const int64_t nr = r->n_reads;
    o->d = *r, o->total_sig = total_sig, o->total_bases = total_bases, o->n_chunks = n_chunks;
    st.add(&o->chunk_read, n_chunks + 1);
    if (mem != RMR_MEM_HOST) return;
#define RMR_DECLARE(field, count) st.add(&o->d.field, (count) + 1);
    if (need_dacs) RMR_DECLARE(dacs, total_sig)
    RMR_READ_ARRAYS(RMR_DECLARE)
#undef RMR_DECLARE
}

// what the fill kernel writes for `nc` chunks (rmr_chunk_fill, rmr_call_read)
struct ChunkSlots {
    float *signal = nullptr;
    int8_t *seqs = nullptr;
    int16_t *maps = nullptr, *lens = nullptr;
    int64_t *rfb = nullptr;
    void declare(Stage &st, int64_t nc, int L, int seq_w, int map_w) {
        st.add(&signal, (size_t)nc * L).add(&seqs, (size_t)nc * seq_w).add(&maps, (size_t)nc * map_w).add(&lens, nc).add(&rfb, nc);
    }
};

}  // namespace rmr

// Copies on the stream of the engine: they expand to RMR_HIP (rmr_internal.h, which the including file brings) on a variable
// `e`, the rmr_engine in scope, and so return from the calling function on an error.  An empty array is skipped.
#define H2D(dst, src, bytes) do { if ((bytes) > 0) RMR_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, e->stream)); } while (0)
#define D2H(dst, src, bytes) do { if ((bytes) > 0) RMR_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, e->stream)); } while (0)
