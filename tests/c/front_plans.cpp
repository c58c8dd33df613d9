// rmr_plan.h on the CPU (tests/test_host_cpu.py): every launch plan of the fp32 conv and front kernels over a sweep of chunk
// lengths, sequence widths, batch sizes, CU counts and register counts stays within the LDS budget it was planned against and
// within the CU's 160 KB; the 11-tap signal front and launch_front's seq_conv1 carve at every chunk length Conv_w_ref admits;
// then the plans of the two benchmark shapes, one line each, for the test to pin.
#include <cstdio>
#include <initializer_list>

#include "rmr_plan.h"

using namespace rmr;

static long checked = 0, bad = 0;

static void check(bool cond, const char *what, int a, int b, long long n) {
    ++checked;
    if (!cond && ++bad <= 20) printf("VIOLATION %s (%d, %d, n %lld)\n", what, a, b, n);
}

// every region of an LDS layout starts on 16 bytes (offsets in 4-byte words)
static bool al4(int words) { return words % 4 == 0; }

// the front plans: the chunk count fits the budget, or ONE chunk takes up to CONV_FRONT_MAX_LDS; the Winograd sig3 form never
// with fewer than three chunks before the small-batch spread
static void check_front(const FrontPlan &p, const char *what, int a, int b, long long n) {
    if (!p.ok) return;
    check(p.lds <= p.budget || (p.cb == 1 && !p.wino && p.lds <= CONV_FRONT_MAX_LDS), what, a, b, n);
    check(p.lds <= PLAN_LDS_CU && p.budget <= PLAN_LDS_CU && p.cb >= 1 && p.cb <= 8 && p.grid >= 1, what, a, b, n);
}

// launch_front's plan of seq_conv1 (k_front.hip): the gather table, then `cb` private carves of five regions in this order, each
// on 16 bytes, none reaching into the next, the last inside the allocation; several chunks per block only within 78 KB (the tap
// kernel: 80 KB), one within the CU's 160 KB
static void check_seq_front(const SeqFrontPlan &p, int kw, int K, int L, int seq_w, int map_w) {
    const int maxlen = map_w - 1, a = kw * 100 + K, b = L * 10000 + maxlen;
    check(p.ok, "front_seq ok", a, b, 0);
    if (!p.ok) return;
    check(p.tap == (kw == 11 && K == 9) || !p.tap, "front_seq tap", a, b, 0);
    check(p.cb >= 1 && p.cb <= 8 && p.fixed == (size_t)kw * K * 80 * 4 && p.fixed % 16 == 0, "front_seq table", a, b, 0);
    check(p.lds == p.fixed + (size_t)p.cb * p.per_chunk * 4 && p.lds <= PLAN_LDS_CU, "front_seq lds", a, b, 0);
    check(p.tap ? p.lds <= 80 * 1024 : (p.cb == 1 || p.lds <= 78 * 1024), "front_seq share", a, b, 0);
    check(al4(p.o_map) && al4(p.o_seq) && al4(p.o_code) && al4(p.o_pidx) && al4(p.o_u) && al4(p.per_chunk), "front_seq align", a, b, 0);
    const int u_words = p.tap ? (maxlen + 1) * 16 : (p.direct ? 0 : (maxlen + 1) * kw * 16);
    check(p.o_map == 0 && p.o_map * 4 + map_w * 2 <= p.o_seq * 4 && p.o_seq * 4 + seq_w <= p.o_code * 4 &&
              p.o_code * 4 + maxlen * (p.tap ? 4 : 8) <= p.o_pidx * 4 && p.o_pidx * 4 + L * 2 <= p.o_u * 4 &&
              p.o_u + u_words <= p.per_chunk, "front_seq regions", a, b, 0);
}

// the smallest max_seq_len (mapping rows of max_seq_len + 1, sequence rows of max_seq_len + K - 1 columns) at which launch_front
// runs fewer than eight chunks per block
static int first_narrow_msl(int kw, int K, int L) {
    for (int msl = 1; msl < 20000; ++msl)
        if (plan_front_seq(kw, K, L, L - kw + 1, msl + K - 1, msl + 1).cb < 8) return msl;
    return -1;
}

static void print_front(const char *name, const FrontPlan &p) {
    printf("%s ok=%d wino=%d cb=%d plane=%d vplane=%d o_v=%d o_front=%d per_chunk=%d o_map=%d o_seq=%d o_code=%d o_pidx=%d o_u=%d "
           "lds=%zu grid=%lld\n", name, p.ok, p.wino, p.cb, p.plane, p.vplane, p.o_v, p.o_front, p.per_chunk, p.o_map, p.o_seq,
           p.o_code, p.o_pidx, p.o_u, p.lds, (long long)p.grid);
}

static void print_conv(const char *name, const ConvPlan &p) {
    printf("%s ok=%d cb=%d nwin=%d pin=%d pout=%d plane=%d lds=%zu grid=%lld\n", name, p.ok, p.cb, p.nwin, p.pin, p.pout, p.plane,
           p.lds, (long long)p.grid);
}

int main() {
    const long long ns[] = {1, 2, 3, 7, 31, 64, 255, 300, 1000, 2047, 4999, 131072, 262144};
    const int cus[] = {256, 80, 32};
    // conv_mfma_kernel: every instantiation (k_conv.hip launch_conv) at the channel counts it runs with
    const int convs[][4] = {{16, 9, 3, 64},  {16, 13, 3, 64}, {128, 5, 1, 64}, {64, 5, 1, 64}, {32, 5, 1, 32}, {16, 11, 1, 32},
                            {32, 9, 3, 64},  {64, 3, 2, 64},  {32, 3, 2, 32},  {16, 5, 1, 16}, {16, 3, 2, 16}};
    for (auto &c : convs)
        for (int pin = 20; pin <= 4000; pin += pin < 400 ? 1 : 11) {
            const int pout = (pin - c[1]) / c[2] + 1, RS = (c[0] / 16) % 2 == 0 ? c[0] / 4 + 4 : c[0] / 4;
            for (int regs = 64; regs <= 256; regs += 16)
                for (int nc : cus)
                    for (long long n : ns) {
                        const ConvPlan p = plan_conv_mfma(c[0], c[1], c[2], c[3], pin, pout, n, nc, regs);
                        if (!p.ok) continue;
                        // the staged rows fit the budget (the plane padding and the trash slot come on top), all of it the CU
                        check((size_t)p.cb * p.pin * RS * 16 <= p.budget && p.lds <= PLAN_LDS_CU, "conv", c[0] * 100 + c[1], pin, n);
                        check(p.nwin == 1 ? p.pin == pin && p.pout == pout : p.cb == 1 && p.pout % 16 == 0 && p.nwin * p.pout >= pout,
                              "conv windows", c[0] * 100 + c[1], pin, n);
                    }
        }
    // the fronts: chunk length L, sig_conv1 width 5 (11: the matrix-core sig3 producer of Conv_w_ref-like shapes)
    for (int L = 20; L <= 4000; L += L < 400 ? 1 : 7)
        for (int kw1 : {5, 11}) {
            const int P1 = L - kw1 + 1, P2 = P1 - kw1 + 1;
            if (P2 < 9) continue;
            const int P3 = (P2 - 9) / 3 + 1, K = 9;
            for (int nc : cus)
                for (long long n : ns) {
                    for (int regs = 64; regs <= 256; regs += 32)
                        for (bool wino : {false, true})
                            check_front(plan_sig3_front_mfma(L, P1, P2, P3, n, nc, wino, regs, regs), "sig3 mfma", L, regs, n);
                    check_front(plan_sig3_front_valu(L, P1, P2, n, nc), "sig3 valu", L, kw1, n);
                    if (kw1 != 5 || (L % 5 && n != 300)) continue;
                    for (int map_w = 2; map_w <= 600; map_w += map_w < 64 ? 1 : 9)
                        for (int seq_w : {map_w + K - 2, map_w + K + 13})
                            for (bool wino : {false, true})
                                check_front(plan_seq2_front(L, P1, P3, K, seq_w, map_w, n, nc, wino), "seq2", L, map_w, n);
                }
        }
    // Conv_w_ref admits the chunk lengths 95 ... 106 (three final positions): the 11-tap signal front on the matrix cores at every
    // one of them - a plan exists in both forms, within its budget, V and the producer scratch on 16 bytes behind the rows and
    // inside the allocation
    for (int L = 95; L <= 106; ++L) {
        const int P1 = L - 10, P2 = P1 - 10, P3 = (P2 - 9) / 3 + 1;
        for (int nc : cus)
            for (long long n : ns)
                for (int regs = 64; regs <= 256; regs += 16)
                    for (bool wino : {false, true}) {
                        const FrontPlan p = plan_sig3_front_mfma(L, P1, P2, P3, n, nc, wino, regs, regs);
                        check(p.ok, "sig3 mfma 11 ok", L, regs, n);
                        check_front(p, "sig3 mfma 11", L, regs, n);
                        check(p.plane >= p.cb * P2 * 4 && al4(p.plane) && al4(p.o_v) && al4(p.o_front) && al4(p.per_chunk) &&
                                  al4(p.vplane) && p.o_v >= 4 * p.plane && p.o_front >= p.o_v + 72 * p.vplane &&
                                  ((size_t)p.o_front + 4 * (size_t)p.per_chunk) * 4 <= p.lds,
                              "sig3 mfma 11 regions", L, regs, n);
                        check(p.per_chunk >= L + 4 * (P1 + 16) && (!p.wino || p.vplane >= p.cb * p.ngrp * 4), "sig3 mfma 11 scratch", L, regs, n);
                    }
    }
    // launch_front's seq_conv1 plan: both tap counts at L = 95 ... 106, the k-mer lengths of tests/test_gpu_kmer_lengths.py, at
    // max_seq_len 20 and at the first max_seq_len of every (kw, K) that runs fewer than eight chunks per block
    const int kmers[] = {1, 2, 3, 6, 8, 9, 10, 11, 13, 21};
    for (int kw : {5, 11})
        for (int L = 95; L <= 106; ++L)
            for (int K : kmers) {
                const int narrow = first_narrow_msl(kw, K, L);
                check(narrow > 1, "front_seq narrow", kw * 100 + K, L, 0);
                for (int msl : {20, narrow - 1, narrow, 2 * narrow}) {
                    const SeqFrontPlan p = plan_front_seq(kw, K, L, L - kw + 1, msl + K - 1, msl + 1);
                    check_seq_front(p, kw, K, L, msl + K - 1, msl + 1);
                    if (!(kw == 11 && K == 9)) check(msl < narrow ? p.cb == 8 : p.cb < 8, "front_seq cb", kw * 100 + K, L * 10000 + msl, 0);
                }
            }
    printf("%ld checks, %ld violations\n", checked, bad);
    // ConvLSTM_w_ref size 64, k-mer 9, 256 CUs: C100 (L 100, 20 bases) and C200 (L 200, 40 bases); the kernels' numRegs on
    // gfx950: sig3_front_wino_kernel<5, 6> 177, sig3_front_mfma_kernel<5, 6> 146, conv_mfma_kernel<16, 9, 3> 110, <16, 13, 3> 126
    for (int L : {100, 200})
        for (long long n : {262144LL, 300LL}) {
            const int P1 = L - 4, P2 = P1 - 4, P3 = (P2 - 9) / 3 + 1, msl = L / 5, seq_w = msl + 8, map_w = msl + 1;
            char name[64];
            snprintf(name, sizeof name, "C%d/%lld sig3_mfma", L, n);
            print_front(name, plan_sig3_front_mfma(L, P1, P2, P3, n, 256, true, 177, 146));
            snprintf(name, sizeof name, "C%d/%lld sig3_valu", L, n);
            print_front(name, plan_sig3_front_valu(L, P1, P2, n, 256));
            snprintf(name, sizeof name, "C%d/%lld seq2", L, n);
            print_front(name, plan_seq2_front(L, P1, P3, 9, seq_w, map_w, n, 256, true));
            snprintf(name, sizeof name, "C%d/%lld seq2_direct", L, n);
            print_front(name, plan_seq2_front(L, P1, P3, 9, seq_w, map_w, n, 256, false));
            snprintf(name, sizeof name, "C%d/%lld sig_conv3", L, n);
            print_conv(name, plan_conv_mfma(16, 9, 3, 64, P2, P3, n, 256, 110));
            snprintf(name, sizeof name, "C%d/%lld seq_conv2", L, n);
            print_conv(name, plan_conv_mfma(16, 13, 3, 64, P1, P3, n, 256, 126));
        }
    // launch_front at L = 100: the first max_seq_len with fewer than eight chunks per block (tests/test_gpu_kmer_lengths.py runs it)
    for (int kw : {5, 11})
        for (int K : {3, 21}) {
            const int msl = first_narrow_msl(kw, K, 100);
            const SeqFrontPlan p = plan_front_seq(kw, K, 100, 100 - kw + 1, msl + K - 1, msl + 1);
            printf("front_seq kw=%d K=%d narrow_msl=%d cb=%d per_chunk=%d lds=%zu\n", kw, K, msl, p.cb, p.per_chunk, p.lds);
        }
    return bad != 0;
}
