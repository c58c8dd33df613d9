// rmr_plan.h on the CPU (tests/test_host_cpu.py): every launch plan of the fp32 conv and front kernels over a sweep of chunk
// lengths, sequence widths, batch sizes, CU counts and register counts stays within the LDS budget it was planned against and
// within the CU's 160 KB; then the plans of the two benchmark shapes, one line each, for the test to pin.
#include <cstdio>
#include <initializer_list>

#include "rmr_plan.h"

using namespace rmr;

static long checked = 0, bad = 0;

static void check(bool cond, const char *what, int a, int b, long long n) {
    ++checked;
    if (!cond && ++bad <= 20) printf("VIOLATION %s (%d, %d, n %lld)\n", what, a, b, n);
}

// the front plans: the chunk count fits the budget, or ONE chunk takes up to CONV_FRONT_MAX_LDS; the Winograd sig3 form never
// with fewer than three chunks before the small-batch spread
static void check_front(const FrontPlan &p, const char *what, int a, int b, long long n) {
    if (!p.ok) return;
    check(p.lds <= p.budget || (p.cb == 1 && !p.wino && p.lds <= CONV_FRONT_MAX_LDS), what, a, b, n);
    check(p.lds <= PLAN_LDS_CU && p.budget <= PLAN_LDS_CU && p.cb >= 1 && p.cb <= 8 && p.grid >= 1, what, a, b, n);
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
    return bad != 0;
}
