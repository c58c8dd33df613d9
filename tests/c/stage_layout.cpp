// rmr_stage.h on the CPU (tests/test_host_cpu.py): layouts committed against a fake engine with a fake base address - every
// slot starts 256-byte aligned, slots do not overlap, the last one ends within the committed total, an empty slot is legal,
// planning again with a larger width (the restart of rmr_call_read) gives a consistent second layout, and the element counts
// rmr_chunk_fill declares for a tiny batch all fit.
#include <algorithm>
#include <cstdio>

#include "rmr_stage.h"

using namespace rmr;

struct FakeEngine {  // what Stage::commit asks of rmr_engine; the growth policy of rmr_engine::ensure
    struct Arena {
        void *ptr = nullptr;
        size_t cap = 0;
    } staging;
    size_t asked = 0;
    int grown = 0;
    int ensure(Arena &a, size_t bytes) {
        asked = bytes;
        if (bytes <= a.cap) return 0;
        a.cap = bytes + bytes / 8;
        a.ptr = reinterpret_cast<void *>((uintptr_t)0x7000000000 + (uintptr_t)0x10000000 * ++grown);  // never dereferenced
        return 0;
    }
};

static int bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

// the invariants of a committed layout; returns the end of the last slot relative to the base
static size_t check_layout(const Stage &st, const FakeEngine &e) {
    const uintptr_t base = (uintptr_t)e.staging.ptr;
    CHECK(e.asked == st.total && st.total <= e.staging.cap);
    size_t end = 0;
    for (const Stage::Slot &s : st.slots) {
        CHECK(s.off % 256 == 0 && (base + s.off) % 256 == 0);
        CHECK(s.off >= end);  // slots come in declaration order: starting at or behind the previous end is not overlapping
        end = s.off + s.bytes;
    }
    CHECK(end <= st.total);
    return end;
}

template <typename T>
static bool holds(const FakeEngine &e, const Stage &st, const T *p, size_t count) {
    const uintptr_t base = (uintptr_t)e.staging.ptr, a = (uintptr_t)p;
    return a >= base && a % 256 == 0 && a + count * sizeof(T) <= base + st.total;
}

int main() {
    {  // mixed types, odd counts, an empty slot in the middle and one at the end
        FakeEngine e;
        Stage st;
        int8_t *a; int16_t *b; float *z; int64_t *c; double *d; uint8_t *z2;
        st.add(&a, 1); st.add(&b, 129); st.add(&z, 0); st.add(&c, 32); st.add(&d, 33); st.add(&z2, 0);
        CHECK(st.commit(&e) == 0);
        CHECK(check_layout(st, e) == 256 + 512 + 256 + 512 && st.total == 256 + 512 + 256 + 512);  // (the empty slot at the end)
        CHECK((uintptr_t)b == (uintptr_t)a + 256 && (uintptr_t)c == (uintptr_t)b + 512 && (void *)z == (void *)c);
        CHECK((uintptr_t)d == (uintptr_t)c + 256 && (uintptr_t)z2 == (uintptr_t)d + 512);
        CHECK(holds(e, st, a, 1) && holds(e, st, b, 129) && holds(e, st, z, 0) && holds(e, st, c, 32) && holds(e, st, d, 33) && holds(e, st, z2, 0));
    }
    {  // nothing but empty slots: a total of 0, the arena is not touched
        FakeEngine e;
        Stage st;
        float *z;
        st.add(&z, 0);
        CHECK(st.commit(&e) == 0 && st.total == 0 && e.grown == 0);
    }
    {  // the layout of rmr_call_read, planned for rows of `cap` bases and again for wider ones: the second layout holds the
       // wider rows, in the same order, in an arena that grew (new base address); a third, narrower plan fits the arena as it is
        FakeEngine e;
        const int64_t ns = 1001, nc = 3;
        const int L = 100, kb = 4, ka = 4;
        float *dsig = nullptr;
        ChunkSlots c;
        size_t total = 0;
        auto plan = [&](int64_t bases) {
            Stage st;
            st.add(&dsig, ns + 4);
            c.declare(st, nc, L, (int)(bases + kb + ka), (int)(bases + 1));
            const int rc = st.commit(&e);
            check_layout(st, e);
            CHECK(st.slots.size() == 6);
            CHECK(holds(e, st, dsig, ns + 4) && holds(e, st, c.signal, nc * L) && holds(e, st, c.seqs, nc * (bases + kb + ka)) &&
                  holds(e, st, c.maps, nc * (bases + 1)) && holds(e, st, c.lens, nc) && holds(e, st, c.rfb, nc));
            CHECK((void *)dsig == e.staging.ptr && (void *)c.signal > (void *)dsig && (void *)c.seqs > (void *)c.signal &&
                  (void *)c.maps > (void *)c.seqs && (void *)c.lens > (void *)c.maps && (void *)c.rfb > (void *)c.lens);
            total = st.total;
            return rc;
        };
        CHECK(plan(208) == 0 && e.grown == 1);
        const size_t t1 = total;
        const void *base1 = e.staging.ptr;
        CHECK(plan(330) == 0 && e.grown == 2 && total > t1 && e.staging.ptr != base1);
        CHECK(plan(208) == 0 && e.grown == 2 && total == t1);
    }
    for (int mem : {RMR_MEM_HOST, RMR_MEM_DEVICE}) {  // rmr_chunk_fill: 2 reads, 3 chunks, L = 8, seq_w = 12, map_w = 5
        FakeEngine e;
        const int64_t nr = 2, ts = 37, tb = 11, nc = 3;
        const int L = 8, seq_w = 12, map_w = 5;
        rmr_reads r{};
        r.n_reads = nr;
        Stage st;
        DevReads dr;
        float *dsig = nullptr;
        int64_t *dgeo = nullptr;
        ChunkSlots c;
        declare_reads(st, &r, mem, false, ts, tb, nc, &dr);
        if (mem == RMR_MEM_HOST) {
            st.add(&dsig, ts + 1);
            st.add(&dgeo, nc * 6);
            c.declare(st, nc, L, seq_w, map_w);
        }
        CHECK(st.commit(&e) == 0);
        check_layout(st, e);
        CHECK(dr.n_chunks == nc && dr.total_sig == ts && dr.total_bases == tb);
        CHECK(holds(e, st, dr.chunk_read, nc + 1));
        if (mem == RMR_MEM_DEVICE) {  // the arrays stay where the caller has them
            CHECK(st.slots.size() == 1 && dr.d.sig_off == nullptr && dr.d.dacs == nullptr);
            continue;
        }
        CHECK(st.slots.size() == 1 + 8 + 2 + 5 && dr.d.dacs == nullptr);  // (the fill kernel does not read the raw signal)
        CHECK(holds(e, st, dr.d.sig_off, nr + 2) && holds(e, st, dr.d.seq_to_sig, tb + nr + 1) && holds(e, st, dr.d.int_seq, tb + 1) &&
              holds(e, st, dr.d.seq_off, nr + 2) && holds(e, st, dr.d.shift, nr + 1) && holds(e, st, dr.d.scale, nr + 1) &&
              holds(e, st, dr.d.focus_bases, nc + 1) && holds(e, st, dr.d.focus_off, nr + 2));
        CHECK(holds(e, st, dsig, ts + 1) && holds(e, st, dgeo, nc * 6) && holds(e, st, c.signal, nc * L) && holds(e, st, c.seqs, nc * seq_w) &&
              holds(e, st, c.maps, nc * map_w) && holds(e, st, c.lens, nc) && holds(e, st, c.rfb, nc));
        // every pointer is a slot of its own
        const void *p[] = {dr.chunk_read, dr.d.sig_off, dr.d.seq_to_sig, dr.d.int_seq, dr.d.seq_off, dr.d.shift, dr.d.scale,
                           dr.d.focus_bases, dr.d.focus_off, dsig, dgeo, c.signal, c.seqs, c.maps, c.lens, c.rfb};
        for (size_t i = 0; i + 1 < sizeof(p) / sizeof(p[0]); ++i) CHECK((uintptr_t)p[i + 1] >= (uintptr_t)p[i] + 256);
        // with the raw signal (rmr_chunk_geometry): one slot more, in front of the offsets
        Stage st2;
        DevReads dr2;
        declare_reads(st2, &r, mem, true, ts, tb, nc, &dr2);
        CHECK(st2.commit(&e) == 0);
        check_layout(st2, e);
        CHECK(st2.slots.size() == 1 + 9 && holds(e, st2, dr2.d.dacs, ts + 1) && (void *)dr2.d.sig_off > (void *)dr2.d.dacs);
    }
    printf("%d failed checks\n", bad);
    return bad ? 1 : 0;
}
