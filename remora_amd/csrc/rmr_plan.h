// Launch plans of the model kernels whose chunk count, LDS image and grid depend on the shape: the fp32 convolutions
// conv_mfma_kernel (k_conv.hip) and the folded fronts sig3_front_* / seq2_front_* (k_conv_front.hip), seq_conv1's carve
// (k_front.hip), the streamed-weight kernels of the networks of more than 64 channels (k_stream.hip, k_stream16.hip) and the
// split-operand convolution (k_conv_bf16s.hip) - chunks per block iteration, LDS layout, dynamic LDS bytes, block size and
// grid, from the model geometry, the batch size, the CU count and (fp32 conv, fronts) the kernel's registers.  Plain integers
// in, a plain struct out, no HIP: the support checks and the launchers call the same function, and so do tests/c/front_plans.cpp
// and tests/c/stream_plans.cpp on the CPU.  A launcher calls its plan, refuses what is not `ok`, fills its argument struct and
// launches.  (Not here: fused_front_plan of k_fused.hip, which writes a device argument struct; kernels with static LDS.)
//
// The common recipe of the fp32 conv and the fronts: blocks per CU from the kernel's registers (512 per SIMD lane, granule 8),
// the LDS budget of a block = its share of the CU's 160 KB at that occupancy, capped at 72 KB (two blocks per CU); the chunk
// count per iteration that fits the budget (and fills its 16-column tiles best); fewer chunks for a small batch; persistent
// blocks, 8 per CU.  The streamed and split kernels plan against fixed budgets; their recipes differ from this one and from
// each other in the ways their sections name.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rmr {

constexpr size_t PLAN_LDS_CU = 160 * 1024;
constexpr size_t PLAN_LDS_BUDGET = 73728;           // 72 KB: two blocks per CU
constexpr size_t CONV_FRONT_MAX_LDS = 156 * 1024;   // what one front block may take of the CU's 160 KB (a long chunk context)

// blocks of `waves` waves each that a CU (4 SIMDs) holds at `regs` registers per lane, clamped to [1, max_blocks]
inline int plan_resident(int regs, int waves, int max_blocks) {
    int wps = 512 / ((regs + 7) & ~7);
    wps = wps < 1 ? 1 : (wps > 8 ? 8 : wps);
    const int r = wps * 4 / waves;
    return r < 1 ? 1 : (r > max_blocks ? max_blocks : r);
}
inline size_t plan_budget(int resident) {
    const size_t share = PLAN_LDS_CU / resident - 512;
    return share < PLAN_LDS_BUDGET ? share : PLAN_LDS_BUDGET;
}
inline double plan_tile_fill(int cols) { return (double)cols / (16.0 * ((cols + 15) / 16)); }
// a small batch (one read per call: a few hundred chunks) spread over the CUs: fewer chunks per iteration until there is a
// block for every CU - a chunk's columns are computed the same way whatever its neighbours in the iteration (same bits), and
// a half-filled tile on an otherwise idle CU costs nothing
inline int plan_spread(int cb, int64_t n, int num_cus) {
    while (cb > 1 && (n + cb - 1) / cb < num_cus) cb = (cb + 1) / 2;
    return cb;
}
// persistent blocks: a grid of several times the resident count evens out the tail
inline int64_t plan_grid(int64_t iters, int num_cus, int per_cu) {
    const int64_t g = (int64_t)num_cus * per_cu;
    return g < iters ? g : iters;
}
// floats per LDS row plane of k chunks of `pin` rows (4 channels a row), and per Winograd V plane of k chunks of `ngrp` groups
inline int plan_plane(int k, int pin) { return ((k * pin * 4) + 63) & ~63; }
inline int plan_vplane(int k, int ngrp) { return ((k * ngrp + 15) & ~15) * 4; }
inline int up4(int words) { return (words + 3) & ~3; }
// floats per row and plane of the four-plane fp32 images (conv_mfma_kernel, k_stream.hip, k_lstm.hip): a quarter of the
// channels, + 4 where that makes row stride / 4 odd (every 16-lane ds_read_b128 group on 16 distinct bank slots)
constexpr int plan_row_stride(int channels) { return (channels / 16) % 2 == 0 ? channels / 4 + 4 : channels / 4; }
// chunks per iteration whose rows of `row_bytes` fit `budget`, 1 .. 8
inline int plan_cb_max(size_t budget, size_t row_bytes) { return budget < row_bytes ? 1 : (budget / row_bytes > 8 ? 8 : (int)(budget / row_bytes)); }
// among the chunk counts cb_max .. (cb_max + 1) / 2, the one whose columns fill their 16-column tiles best (Conv_w_ref's
// merge_conv1: 4 x 20 columns = 5 tiles exactly, where 5 chunks would pad the 7th tile to 25 %); ties go to the larger count
inline int plan_best_cb(int cb_max, int pout) {
    int cb = cb_max;
    double best = -1.0;
    for (int k = cb_max; k >= (cb_max + 1) / 2; --k) {
        const double eff = plan_tile_fill(k * pout);
        if (eff > best + 1e-9) { best = eff; cb = k; }
    }
    return cb;
}

// ---- conv_mfma_kernel<IC, KW, STRIDE> of `oc` output channels (k_conv.hip); conv_stream_kernel<KW, STRIDE> (k_stream.hip) ----
struct ConvPlan {
    bool ok = false;
    int nw = 0, cb = 0;          // waves per block (conv_stream_kernel); chunks per iteration (1 with windows)
    int nwin = 1, pin = 0, pout = 0;  // position windows: rows staged / columns computed per window (the chunk's when nwin == 1)
    int rs = 0, plane = 0;       // floats per row and plane; LDS plane stride in floats
    size_t budget = 0, lds = 0;  // the block's LDS share; dynamic LDS bytes (0: not even one window fits the share)
    int64_t grid = 0;
};

// a chunk whose rows do not fit goes through position windows: the most output positions whose input rows ((win - 1) * stride
// + kw of them) fit `budget`, whole column tiles, one window of one chunk per iteration.  false: fewer than 16 columns fit
inline bool plan_windows(ConvPlan &p, int kw, int stride, int pout) {
    const int rows_fit = (int)(p.budget / ((size_t)p.rs * 4 * sizeof(float)));
    p.pout = (rows_fit - kw) / stride + 1;
    if (p.pout < 16) return false;
    p.pout &= ~15;
    p.nwin = (pout + p.pout - 1) / p.pout;
    p.pin = (p.pout - 1) * stride + kw;
    p.cb = 1;
    return true;
}
// the image of p.cb x p.pin rows: four planes + the trash slot for masked staging writes; the grid over its iterations
inline void plan_conv_image(ConvPlan &p, int64_t n, int num_cus, int per_cu) {
    p.plane = ((p.cb * p.pin * p.rs) + 63) & ~63;
    p.lds = (size_t)p.plane * 4 * sizeof(float) + 64;
    p.grid = plan_grid(p.nwin > 1 ? n * p.nwin : (n + p.cb - 1) / p.cb, num_cus, per_cu);
}

inline ConvPlan plan_conv_mfma(int ic, int kw, int stride, int oc, int pin, int pout, int64_t n, int num_cus, int regs) {
    ConvPlan p;
    p.rs = plan_row_stride(ic);
    p.budget = plan_budget(plan_resident(regs, oc / 16, 8));
    const size_t row_bytes = (size_t)pin * p.rs * 4 * sizeof(float);  // all four planes
    p.cb = plan_spread(plan_best_cb(plan_cb_max(p.budget, row_bytes), pout), n, num_cus);
    p.pin = pin; p.pout = pout;
    if (row_bytes > p.budget && !plan_windows(p, kw, stride, pout)) return p;
    plan_conv_image(p, n, num_cus, 8 * (oc >= 64 ? 1 : 64 / oc));
    p.ok = p.lds <= PLAN_LDS_CU;
    return p;
}

// ---- the streamed-weight kernels (k_stream.hip fp32, k_stream16.hip bf16 / f16): channel counts are runtime values ----
constexpr size_t STREAM_BUDGET = 65536;                // rows of several chunks: two blocks per CU
constexpr size_t STREAM_MAX_LDS = 160 * 1024 - 256;    // what one block may take
constexpr size_t STREAM_WINDOW_ABOVE = 150 * 1024;     // fp32 conv: a chunk of more staged bytes (+ trash slot) goes through windows
constexpr int STREAM_GRID_PER_CU = 4;

// waves per block of both streamed convolutions: one output-channel tile each where that is at most 8, else the largest divisor
// of the tile count in 8 .. 4 (equal work), else 8
inline int plan_stream_waves(int oc) {
    const int ot = oc / 16;
    for (int d = 8; ot > 8 && d >= 4; --d)
        if (ot % d == 0) return d;
    return ot < 8 ? ot : 8;
}

// conv_stream_kernel: no spreading of a small batch; ONE chunk may take up to STREAM_WINDOW_ABOVE, a longer one goes through
// windows sized against STREAM_BUDGET
inline ConvPlan plan_conv_stream(int ic, int oc, int kw, int stride, int pin, int pout, int64_t n, int num_cus) {
    ConvPlan p;
    p.nw = plan_stream_waves(oc);
    p.rs = plan_row_stride(ic);
    p.budget = STREAM_BUDGET;
    const size_t row_bytes = (size_t)pin * p.rs * 4 * sizeof(float);  // all four planes
    p.cb = plan_best_cb(plan_cb_max(p.budget, row_bytes), pout);
    p.pin = pin; p.pout = pout;
    if (row_bytes + 64 > STREAM_WINDOW_ABOVE && !plan_windows(p, kw, stride, pout)) return p;
    plan_conv_image(p, n, num_cus, STREAM_GRID_PER_CU);
    p.ok = p.lds <= STREAM_MAX_LDS;
    return p;
}

// conv_stream16_kernel: flat rows of 16-bit channels + 16 bytes (row bytes / 16 odd); an iteration's image is its chunks' rows
// + the rows a padded k-step and a clamped column may touch.  No windows: a chunk that does not fit is refused
struct Conv16Plan {
    bool ok = false;
    int nw = 0, cb = 0, rb = 0, ks = 0;  // waves per block; chunks per iteration; LDS row bytes; k-steps of 32
    size_t lds = 0;                      // dynamic LDS bytes, whole 16-byte pieces (the kernel zero-fills them)
    int64_t grid = 0;
};
inline int plan_row_bytes16(int channels) { return channels * 2 + 16; }
inline size_t plan_conv_stream16_lds(int ic, int kw, int pin, int cb) { return ((size_t)cb * pin + kw + 2) * plan_row_bytes16(ic); }

inline Conv16Plan plan_conv_stream16(int ic, int oc, int kw, int pin, int pout, int64_t n, int num_cus) {
    Conv16Plan p;
    p.nw = plan_stream_waves(oc);
    p.rb = plan_row_bytes16(ic);
    p.ks = (kw * ic + 31) / 32;
    p.cb = plan_spread(plan_best_cb(plan_cb_max(STREAM_BUDGET, (size_t)pin * p.rb), pout), n, num_cus);
    p.lds = (plan_conv_stream16_lds(ic, kw, pin, p.cb) + 15) & ~(size_t)15;
    p.grid = plan_grid((n + p.cb - 1) / p.cb, num_cus, STREAM_GRID_PER_CU);
    p.ok = p.lds <= STREAM_MAX_LDS;  // (cb > 1 always fits: several chunks' rows stay within STREAM_BUDGET)
    return p;
}

// lstm_stream_kernel / lstm_stream16_kernel: H / 16 waves x 16 nt chunks per group, two x and two h images.  Four column tiles
// per wave halve the weight traffic of two, and fit (registers: 512 threads; LDS) up to 128 units
struct LstmStreamPlan {
    bool ok = false;
    int nt = 0, threads = 0, bound = 0;  // column tiles per wave; block size 4 H; the instantiation's launch bound
    int rs = 0, rb = 0, ksh = 0;         // fp32: floats per row and plane;  16-bit: row bytes, k-steps of 32
    size_t lds = 0;
    int64_t grid = 0;
};
inline LstmStreamPlan plan_lstm_streamed(int H, int64_t n, int num_cus, bool half) {
    LstmStreamPlan p;
    p.nt = H <= 128 ? 4 : 2;
    p.bound = H <= 128 ? 512 : 1024;
    p.threads = 4 * H;
    p.rs = plan_row_stride(H);
    p.rb = plan_row_bytes16(H);
    p.ksh = H / 32;
    p.lds = (size_t)4 * 16 * p.nt * (half ? p.rb : 4 * p.rs * sizeof(float));  // 4 images of 16 nt rows (fp32: in 4 planes)
    p.grid = plan_grid((n + 16 * p.nt - 1) / (16 * p.nt), num_cus, STREAM_GRID_PER_CU);
    // 16-bit: the fc partial sums [H / 16][16 nt][16] floats take the place of the two h images
    p.ok = p.lds <= STREAM_MAX_LDS && (!half || (size_t)H * 16 * p.nt * 4 <= p.lds / 2);
    return p;
}
inline LstmStreamPlan plan_lstm_stream(int H, int64_t n, int num_cus) { return plan_lstm_streamed(H, n, num_cus, false); }
inline LstmStreamPlan plan_lstm_stream16(int H, int64_t n, int num_cus) { return plan_lstm_streamed(H, n, num_cus, true); }

// ---- conv_bf16s_kernel<IC, ..., NP> (k_conv_bf16s.hip): `nparts` images of 16-byte slots (8 channels), 2 planes (ic 16: two
// taps per k-step) or 4; whole groups of four chunks from 4 up; no spreading; 2 blocks per CU ----
constexpr size_t SPLIT_BUDGET = 112 * 1024;
struct SplitPlan {
    bool ok = false;
    int cb = 0, plane = 0, part = 0;  // chunks per iteration; plane / part stride in slots
    size_t lds = 0;
    int64_t grid = 0;
};
inline SplitPlan plan_conv_split(int ic, int pin, int nparts, int64_t n, int num_cus) {
    SplitPlan p;
    const int ks = ic == 16 ? 1 : ic / 32, slr = ks % 2 == 0 ? ks + 1 : ks, planes = ic == 16 ? 2 : 4;  // slr: odd row stride in slots
    p.cb = plan_cb_max(SPLIT_BUDGET, (size_t)pin * slr * 16 * planes * nparts);
    if (p.cb >= 4) p.cb &= ~3;
    p.plane = ((p.cb * pin + 2) * slr + 15) & ~15;  // + 2 guard rows
    p.part = planes * p.plane + 16;                 // + trash slot
    p.lds = (size_t)p.part * nparts * 16;
    p.grid = plan_grid((n + p.cb - 1) / p.cb, num_cus, 2);
    p.ok = p.lds <= PLAN_LDS_CU;
    return p;
}

// ---- the folded fronts (k_conv_front.hip): 4 waves, 64 output channels, 16 input channels (4 floats per row and plane) ----
struct FrontPlan {
    bool ok = false;
    bool wino = false;       // the Winograd kernel (sig3_front_wino_kernel / seq2_front_wino_kernel)
    int cb = 0;              // chunks per iteration
    int plane = 0;           // floats per row plane
    int vplane = 0, o_v = 0; // Winograd: floats per V plane, LDS offset of V
    int o_front = 0;         // LDS offset of the producer scratch
    int per_chunk = 0;       // producer scratch per chunk (sig3 matrix-core producer: per wave)
    int o_map = 0, o_seq = 0, o_code = 0, o_pidx = 0, o_u = 0;  // seq2: offsets inside a chunk's scratch
    int ngrp = 0;            // groups of four output positions per chunk (the Winograd forms)
    size_t budget = 0;       // the LDS budget the chunk count was chosen against (one chunk may exceed it: CONV_FRONT_MAX_LDS)
    size_t lds = 0;          // dynamic LDS bytes
    int64_t grid = 0;
};

inline void plan_finish(FrontPlan &p, int64_t n, int num_cus) {
    p.grid = plan_grid((n + p.cb - 1) / p.cb, num_cus, 8);
    p.ok = true;
}

// sig_conv1 -> sig_conv2 (matrix cores) -> sig_conv3 (sig3_front_mfma_kernel / sig3_front_wino_kernel).  `wino`: the
// Winograd form is allowed; it is taken where at least three chunks per iteration fit (with fewer, three of the four producing
// waves idle: C200, 4.5 against the direct form's 3.1 ms per 250 k chunks).  The direct form takes one chunk past the 72 KB
// budget (long chunk contexts), up to CONV_FRONT_MAX_LDS.
inline void plan_sig3_mfma_layout(FrontPlan &p, int k, int P2) {
    p.plane = plan_plane(k, P2);
    p.vplane = p.wino ? plan_vplane(k, p.ngrp) : 0;
    p.o_v = 4 * p.plane + 16;
    p.o_front = p.o_v + 72 * p.vplane;  // V = 6 points x 12 (phase, plane) planes
    p.lds = ((size_t)p.o_front + 4 * (size_t)p.per_chunk) * sizeof(float);
}

inline FrontPlan plan_sig3_front_mfma(int L, int P1, int P2, int P3, int64_t n, int num_cus, bool wino, int regs_wino,
                                      int regs_direct) {
    FrontPlan p;
    p.per_chunk = ((L + 3) & ~3) + 4 * ((P1 + 16 + 3) & ~3);
    p.ngrp = (P3 + 3) / 4;
    for (p.wino = wino;; p.wino = false) {
        int resident = plan_resident(p.wino ? regs_wino : regs_direct, 4, 4);
        if (p.wino && resident > 2) resident = 2;  // V is 1.5 x the rows: four chunks per iteration need a half CU's LDS
        const size_t budget = p.budget = plan_budget(resident);
        // score of a chunk count = tile fill of the matrix phase x balance of the producer phase (4 waves, one chunk at a time),
        // never below half of the largest count that fits
        int cb_max = 0, cb = 0;
        double best = -1.0;
        for (int k = 8; k >= 1; --k) {
            plan_sig3_mfma_layout(p, k, P2);
            if (p.lds > budget && !(k == 1 && !p.wino && p.lds <= CONV_FRONT_MAX_LDS)) continue;
            if (cb_max == 0) cb_max = k;
            if (2 * k < cb_max) break;
            const double score = plan_tile_fill(p.wino ? k * p.ngrp : k * P3) * (double)k / (4.0 * ((k + 3) / 4));
            if (score > best + 1e-9) { best = score; cb = k; }
        }
        if (cb_max == 0 || (p.wino && cb < 3)) {
            if (p.wino) continue;
            return p;  // one chunk does not fit
        }
        p.cb = plan_spread(cb, n, num_cus);
        plan_sig3_mfma_layout(p, p.cb, P2);
        plan_finish(p, n, num_cus);
        return p;
    }
}

// the same with the VALU producers (sig3_front_kernel): the largest chunk count within 72 KB, else one chunk per iteration up
// to CONV_FRONT_MAX_LDS; no spreading of small batches
inline FrontPlan plan_sig3_front_valu(int L, int P1, int P2, int64_t n, int num_cus) {
    FrontPlan p;
    p.per_chunk = up4(((L + 3) & ~3) + P1 * 4);
    p.budget = PLAN_LDS_BUDGET;
    for (p.cb = 8; p.cb >= 1; --p.cb) {
        p.plane = plan_plane(p.cb, P2);
        p.o_front = 4 * p.plane + 16;
        p.lds = ((size_t)p.o_front + (size_t)p.cb * p.per_chunk) * sizeof(float);
        if (p.lds <= p.budget || p.cb == 1) break;
    }
    if (p.lds > CONV_FRONT_MAX_LDS) return p;
    plan_finish(p, n, num_cus);
    return p;
}

// seq_conv1 (the gather-sum) -> seq_conv2 (seq2_front_kernel / seq2_front_wino_kernel).  `wino`: the polyphase Winograd form
// is allowed; it is taken where at least three chunks per iteration fit a half CU with V in the place of the gather table and
// the scratch.  The direct form: the largest chunk count within 72 KB, else one chunk up to CONV_FRONT_MAX_LDS.
inline FrontPlan plan_seq2_front(int L, int P1, int P3, int K, int seq_w, int map_w, int64_t n, int num_cus, bool wino) {
    FrontPlan p;
    const int maxlen = map_w - 1, wt_words = 5 * K * 80;  // wt_words: the gather table
    int off = 0;
    p.o_map = off; off += up4((map_w * 2 + 3) / 4);
    p.o_seq = off; off += up4((seq_w + 3) / 4);
    p.o_code = off; off += up4(maxlen * 2);
    p.o_pidx = off; off += up4((L * 2 + 3) / 4);
    p.o_u = off; off += (maxlen + 1) * 5 * 16;
    p.per_chunk = up4(off);
    if (wino) {
        p.ngrp = (P3 + 3) / 4;
        auto layout = [&](int k) {
            p.plane = plan_plane(k, P1);
            p.vplane = plan_vplane(k, p.ngrp);
            p.o_front = p.o_v = 4 * p.plane + 16;
            const size_t front = (size_t)wt_words + (size_t)k * p.per_chunk, v = (size_t)96 * p.vplane;
            p.lds = ((size_t)p.o_front + (front > v ? front : v)) * sizeof(float);
        };
        int k = 8;
        for (; k >= 3; --k) {
            layout(k);
            if (p.lds <= (size_t)80 * 1024 - 512) break;
        }
        if (k >= 3) {
            p.wino = true;
            p.budget = (size_t)80 * 1024 - 512;
            p.cb = plan_spread(k, n, num_cus);
            layout(p.cb);
            plan_finish(p, n, num_cus);
            return p;
        }
        // (the direct kernel reads neither vplane nor o_v: they keep what the three-chunk trial left)
    }
    auto layout = [&](int k) {
        p.plane = plan_plane(k, P1);
        p.o_front = 4 * p.plane + 16;
        p.lds = ((size_t)p.o_front + wt_words + (size_t)k * p.per_chunk) * sizeof(float);
    };
    p.budget = PLAN_LDS_BUDGET;
    int k = 8;
    for (; k > 1; --k) {
        layout(k);
        if (p.lds <= p.budget) break;
    }
    p.cb = plan_spread(k, n, num_cus);
    layout(p.cb);
    if (p.lds > CONV_FRONT_MAX_LDS) return p;
    plan_finish(p, n, num_cus);
    return p;
}

// ---- seq_conv1 alone from the chunk arrays (k_front.hip, launch_front): the gather table of kw x K x 5 rows, then a private
// carve per chunk - mapping row, sequence row, window codes, base-of-position row and (two-level forms) the per-base table U ----
struct SeqFrontPlan {
    bool ok = false;
    bool tap = false;     // front_seq_tap_kernel<11, 9>: one wave per chunk, `cb` waves per block
    bool direct = false;  // front_seq_kernel<11, true>: no U table
    int cb = 0;           // chunks per block (32 threads each; tap: 64)
    int o_map = 0, o_seq = 0, o_code = 0, o_pidx = 0, o_u = 0, per_chunk = 0;  // in 4-byte words, every region 16-byte aligned
    size_t fixed = 0;     // bytes of the gather table in front of the chunks' carves
    size_t lds = 0;       // dynamic LDS bytes
};

inline SeqFrontPlan plan_front_seq(int kw, int K, int L, int P1, int seq_w, int map_w) {
    SeqFrontPlan p;
    const int maxlen = map_w - 1;
    p.fixed = (size_t)kw * K * 80 * 4;
    // Conv_w_ref's released shape (11 taps, k-mer length 9): the tap-by-tap two-level kernel, one wave per chunk, 32-bit window
    // codes and one tap's U rows; two blocks (16 waves) per CU, longer rows go on to the forms below
    if (kw == 11 && K == 9 && P1 * 4 <= 64 * 6 && maxlen <= 1024) {
        int off = 0;
        p.o_map = off; off += up4((map_w * 2 + 3) / 4);
        p.o_seq = off; off += up4((seq_w + 3) / 4);
        p.o_code = off; off += up4(maxlen);
        p.o_pidx = off; off += up4((L * 2 + 3) / 4);
        p.o_u = off; off += (maxlen + 1) * 16;
        p.per_chunk = up4(off);
        p.cb = 8;
        p.lds = p.fixed + (size_t)p.cb * p.per_chunk * 4;
        if (p.lds <= 80 * 1024) {
            p.tap = p.ok = true;
            return p;
        }
    }
    p.direct = kw == 11;
    int off = 0;
    p.o_map = off; off += up4((map_w * 2 + 3) / 4);
    p.o_seq = off; off += up4((seq_w + 3) / 4);
    p.o_code = off; off += up4(maxlen * 2);
    p.o_pidx = off; off += up4((L * 2 + 3) / 4);
    p.o_u = off; if (!p.direct) off += (maxlen + 1) * kw * 16;
    p.per_chunk = up4(off);
    // eight chunks per block, halved until the block fits 78 KB (two blocks per CU); one chunk may take the CU's 160 KB
    const size_t lds_cap = (size_t)78 * 1024;
    p.cb = 8;
    while (p.cb > 1 && p.fixed + (size_t)p.cb * p.per_chunk * 4 > lds_cap) p.cb >>= 1;
    p.lds = p.fixed + (size_t)p.cb * p.per_chunk * 4;
    p.ok = p.lds <= PLAN_LDS_CU;
    return p;
}

}  // namespace rmr
