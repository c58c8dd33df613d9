// rmr_plan.h on the CPU (tests/test_host_stream_cases.py): the launch plans of the streamed-weight kernels (k_stream.hip,
// k_stream16.hip) and of the split convolution (k_conv_bf16s.hip).  Part a: over ConvLSTM_w_ref at every size 80 .. 256, every
// chunk length 29 .. 470, nine batch sizes and three CU counts, every plan that is `ok` keeps the invariants its kernel relies
// on (the limits are restated here, not read from the header).  Part b: one line per plan, for the test to hold the Python
// restatement (tests/stream_cases.py, tests/test_gpu_split_shapes.py) to.  A plan's n and CU count enter the fp32 convolutions,
// the LSTMs and the split convolution through the grid alone, which the restatement does not have: their lines are printed once
// per shape; the 16-bit convolutions spread a small batch, so theirs are printed per (n, CUs).
#include <cstdio>
#include <initializer_list>

#include "rmr_plan.h"

using namespace rmr;

static long checked = 0, bad = 0;

static void check(bool cond, const char *what, int a, int b, long long n) {
    ++checked;
    if (!cond && ++bad <= 20) printf("VIOLATION %s (%d, %d, n %lld)\n", what, a, b, n);
}

constexpr size_t kMaxLds = 160 * 1024 - 256, kBudget = 65536, kSplitBudget = 112 * 1024, kSplitMaxLds = 160 * 1024;

struct Layer { const char *name; int ic, oc, kw, stride, pin, pout; };

static bool waves_ok(int nw, int oc) { return nw >= 1 && nw <= 8 && ((oc / 16) % nw == 0 || nw == 8); }
static bool grid_ok(int64_t grid, int64_t iters, int cus, int per_cu) { return grid >= 1 && grid <= iters && grid <= (int64_t)cus * per_cu; }

static void check_conv(const Layer &l, int L, long long n, int cus) {
    const ConvPlan p = plan_conv_stream(l.ic, l.oc, l.kw, l.stride, l.pin, l.pout, n, cus);
    const int a = l.ic * 100 + l.kw;
    check(p.ok, "conv ok", a, L, n);  // windows keep every chunk length in
    if (!p.ok) return;
    check(p.lds <= kMaxLds && p.lds >= (size_t)p.cb * p.pin * p.rs * 16 + 64, "conv lds", a, L, n);
    check(p.rs >= l.ic / 4 && p.rs % 4 == 0 && (p.rs / 4) % 2 == 1, "conv row stride", a, L, n);
    check(p.cb >= 1 && p.cb <= 8 && (p.cb == 1 || (size_t)p.cb * p.pin * p.rs * 16 <= kBudget), "conv budget", a, L, n);
    if (p.nwin > 1) {
        check(p.cb == 1 && p.pout % 16 == 0 && p.nwin * p.pout >= l.pout && (p.nwin - 1) * p.pout < l.pout &&
                  p.pin == (p.pout - 1) * l.stride + l.kw, "conv windows", a, L, n);
        check((size_t)p.pin * p.rs * 16 <= kBudget, "conv window budget", a, L, n);
    } else {
        check(p.pin == l.pin && p.pout == l.pout, "conv whole chunks", a, L, n);
    }
    check(waves_ok(p.nw, l.oc), "conv waves", a, L, n);
    check(grid_ok(p.grid, p.nwin > 1 ? n * p.nwin : (n + p.cb - 1) / p.cb, cus, 4), "conv grid", a, L, n);
}

static void check_conv16(const Layer &l, int L, long long n, int cus) {
    const Conv16Plan p = plan_conv_stream16(l.ic, l.oc, l.kw, l.pin, l.pout, n, cus);
    const int a = l.ic * 100 + l.kw;
    // one chunk's image is what check_conv_stream16 asks for, and the only one a plan is refused for
    check(p.ok == (plan_conv_stream16_lds(l.ic, l.kw, l.pin, 1) <= kMaxLds), "conv16 ok", a, L, n);
    if (!p.ok) return;
    check(p.lds <= kMaxLds && p.lds % 16 == 0 && p.lds >= ((size_t)p.cb * l.pin + l.kw + 2) * p.rb, "conv16 lds", a, L, n);
    check(p.rb == 2 * l.ic + 16 && (p.rb / 16) % 2 == 1 && p.ks * 32 >= l.kw * l.ic && (p.ks - 1) * 32 < l.kw * l.ic, "conv16 rows", a, L, n);
    check(p.cb >= 1 && p.cb <= 8 && (p.cb == 1 || (size_t)p.cb * l.pin * p.rb <= kBudget), "conv16 budget", a, L, n);
    check(p.cb == 1 || (n + p.cb - 1) / p.cb >= cus, "conv16 spread", a, L, n);
    check(waves_ok(p.nw, l.oc), "conv16 waves", a, L, n);
    check(grid_ok(p.grid, (n + p.cb - 1) / p.cb, cus, 4), "conv16 grid", a, L, n);
}

static void check_lstm(const LstmStreamPlan &p, bool half, int H, long long n, int cus) {
    check(p.ok, "lstm ok", H, half, n);
    if (!p.ok) return;
    check(p.lds <= kMaxLds, "lstm lds", H, half, n);
    check(p.threads == 4 * H && p.threads <= p.bound && p.nt == (H <= 128 ? 4 : 2) && p.bound == (H <= 128 ? 512 : 1024), "lstm block", H, half, n);
    if (half) {
        check(p.rb == 2 * H + 16 && p.ksh * 32 == H && p.lds == (size_t)4 * 16 * p.nt * p.rb, "lstm16 images", H, half, n);
        check((size_t)H * 16 * p.nt * 4 <= p.lds / 2, "lstm16 fc partial sums", H, half, n);
    } else {
        check(p.rs >= H / 4 && (p.rs / 4) % 2 == 1 && p.lds == (size_t)16 * 16 * p.nt * p.rs * 4, "lstm images", H, half, n);
        check((size_t)H * 16 * p.nt * 4 <= p.lds / 2, "lstm fc partial sums", H, half, n);
    }
    check(grid_ok(p.grid, (n + 16 * p.nt - 1) / (16 * p.nt), cus, 4), "lstm grid", H, half, n);
}

static void check_split(int ic, int pin, int parts, long long n, int cus) {
    const SplitPlan p = plan_conv_split(ic, pin, parts, n, cus);
    if (!p.ok) return;
    const int ks = ic == 16 ? 1 : ic / 32, slr = ks | 1, planes = ic == 16 ? 2 : 4, a = ic * 10 + parts;
    check(p.lds <= kSplitMaxLds && p.lds == (size_t)p.part * parts * 16, "split lds", a, pin, n);
    check(p.plane % 16 == 0 && p.plane >= (p.cb * pin + 2) * slr && p.part == planes * p.plane + 16, "split image", a, pin, n);
    check(p.cb >= 1 && p.cb <= 8 && (p.cb < 4 || p.cb % 4 == 0) &&
              (p.cb == 1 || (size_t)p.cb * pin * slr * 16 * planes * parts <= kSplitBudget), "split budget", a, pin, n);
    check(grid_ok(p.grid, (n + p.cb - 1) / p.cb, cus, 2), "split grid", a, pin, n);
}

int main() {
    const int cus_list[] = {256, 304, 80};
    for (int pass = 0; pass < 2; ++pass) {  // 0: part a, then the count; 1: part b
        for (int size = 80; size <= 256; size += 16) {
            for (int L = 29; L <= 470; ++L) {
                const int P1 = L - 4, P2 = P1 - 4, P3 = (P2 - 9) / 3 + 1, T = P3 - 4;
                const Layer layers[] = {{"sig_conv3", 16, size, 9, 3, P2, P3}, {"seq_conv2", 16, size, 13, 3, P1, P3},
                                        {"merge_conv1", 2 * size, size, 5, 1, P3, T}};
                if (pass == 1)
                    for (const Layer &l : layers) {
                        const ConvPlan p = plan_conv_stream(l.ic, l.oc, l.kw, l.stride, l.pin, l.pout, 1, 256);
                        printf("conv32 %d %d %s %d %d %d %d %d %d %d %zu\n", size, L, l.name, p.ok, p.nw, p.cb, p.nwin, p.pin, p.pout, p.rs, p.lds);
                    }
                for (int cus : cus_list) {
                    const long long ns[] = {1, 3, 5, 37, 64, 300, 1061, 1500, 8LL * cus + 37};
                    for (long long n : ns)
                        for (const Layer &l : layers) {
                            if (pass == 0) {
                                check_conv(l, L, n, cus);
                                check_conv16(l, L, n, cus);
                            } else {
                                const Conv16Plan p = plan_conv_stream16(l.ic, l.oc, l.kw, l.pin, l.pout, n, cus);
                                printf("conv16 %d %d %lld %d %s %d %d %d %zu\n", size, L, n, cus, l.name, p.ok, p.nw, p.cb, p.lds);
                            }
                        }
                }
            }
            for (int cus : cus_list) {
                const long long ns[] = {1, 3, 5, 37, 64, 300, 1061, 1500, 8LL * cus + 37};
                for (long long n : ns) {
                    if (pass == 1) continue;
                    check_lstm(plan_lstm_stream(size, n, cus), false, size, n, cus);
                    if (size % 32 == 0) check_lstm(plan_lstm_stream16(size, n, cus), true, size, n, cus);  // what launch_lstm_stream16 takes
                }
            }
            if (pass == 1) {
                const LstmStreamPlan p = plan_lstm_stream(size, 1, 256), h = plan_lstm_stream16(size, 1, 256);
                printf("lstm32 %d %d %d %d %zu\n", size, p.ok, p.nt, p.threads, p.lds);
                if (size % 32 == 0) printf("lstm16 %d %d %d %d %zu\n", size, h.ok, h.nt, h.threads, h.lds);
            }
        }
        for (int ic : {16, 64, 128})
            for (int pin = 10; pin <= 600; ++pin)
                for (int parts = 1; parts <= 3; ++parts) {
                    if (pass == 1) {
                        const SplitPlan p = plan_conv_split(ic, pin, parts, 1, 256);
                        printf("split %d %d %d %d %d %zu\n", ic, pin, parts, p.ok, p.cb, p.lds);
                        continue;
                    }
                    for (int cus : cus_list)
                        for (long long n : {1LL, 3LL, 5LL, 37LL, 64LL, 300LL, 1061LL, 1500LL, 8LL * cus + 37})
                            check_split(ic, pin, parts, n, cus);
                }
        if (pass == 0) printf("%ld checks, %ld violations\n", checked, bad);
    }
    return bad != 0;
}
