"""The case table of tests/test_gpu_stream_shapes.py and the launch plans of the streamed-weight kernels, restated.

Networks of more than 64 channels run on conv_stream_kernel / lstm_stream_kernel (k_stream.hip, fp32) and conv_stream16_kernel /
lstm_stream16_kernel (k_stream16.hip, bf16 and f16).  Which form of those kernels a launch takes - waves per block, chunks per
block iteration (cb), position windows, the column tiles of a work item (NTV), LDS bytes - is decided on the host by
plan_conv_stream, plan_lstm_stream, plan_conv_stream16 and plan_lstm_stream16 (remora_amd/csrc/rmr_plan.h), which the launchers
call.  The functions below restate that arithmetic in the way conv_split_plan (tests/test_gpu_split_shapes.py) restates
plan_conv_split, so that tests/test_host_stream_cases.py can assert without a GPU, and the GPU tests use where nothing is
compiled, that every case takes the path it is there for.  The restatement is held to the launch code by
test_stream_plans_keep_their_invariants_and_the_restatement_follows_them (tests/test_host_stream_cases.py): it runs the header's
plans on the CPU over every size, chunk length and batch of the case tables and compares every number with the functions here.
When it fails after a change of the plans, change them here, and look at the case table again - a case may no longer reach its
path.

A plain module (no tests in it), like duplex_fixture.py."""
from collections import namedtuple

LDS_LIMIT = 160 * 1024 - 256   # what every launcher admits
WINDOW_ABOVE = 150 * 1024      # launch_conv_stream_t: a chunk of more staged bytes (+ 64) goes through position windows
BUDGET = 65536                 # two blocks per CU
CONV_NT = 4                    # kConvStreamNT: column tiles per work item


def layer_rows(L):
    """Rows of sig_conv1 / seq_conv1 (P1), sig_conv2 (P2), sig_conv3 / seq_conv2 (P3) and merge_conv1 = LSTM steps (T)."""
    P1 = L - 4
    P2 = P1 - 4
    P3 = (P2 - 9) // 3 + 1
    assert (P1 - 13) // 3 + 1 == P3
    return P1, P2, P3, P3 - 4


def conv_layers(size, L):
    """{layer: (ic, oc, kw, stride, pin, pout)} of the three streamed convolutions of ConvLSTM_w_ref at kernel size `size`."""
    P1, P2, P3, T = layer_rows(L)
    return {"sig_conv3": (16, size, 9, 3, P2, P3), "seq_conv2": (16, size, 13, 3, P1, P3), "merge_conv1": (2 * size, size, 5, 1, P3, T)}


def waves(oc):
    """Waves per block of both convolution launchers: one per output tile up to 8, else the largest divisor in 8 .. 4, else 8."""
    ot = oc // 16
    if ot <= 8:
        return ot
    for d in range(8, 3, -1):
        if ot % d == 0:
            return d
    return 8


def _best_cb(cb_max, pout):
    """The chunk count in cb_max .. (cb_max + 1) / 2 whose columns fill their 16-column tiles best (the largest on a tie)."""
    cb, best = cb_max, -1.0
    for k in range(cb_max, (cb_max + 1) // 2 - 1, -1):
        cols = k * pout
        eff = cols / (16.0 * ((cols + 15) // 16))
        if eff > best + 1e-9:
            best, cb = eff, k
    return cb


ConvPlan = namedtuple("ConvPlan", "nw uneven cb nwin pin_w pout_w last_cols rs lds")


def conv_stream_plan(ic, oc, kw, stride, pin, pout):
    """launch_conv_stream_t (k_stream.hip).  `uneven`: the block's waves do not share the output tiles of a tile group equally;
    nwin > 1: one window of pout_w columns (pin_w rows) of one chunk per iteration, the last window `last_cols` columns."""
    g = ic // 16
    rs = ic // 4 + 4 if g % 2 == 0 else ic // 4
    nw = waves(oc)
    row_bytes = pin * rs * 16
    cb = _best_cb(max(1, min(8, BUDGET // row_bytes)), pout)
    nwin, pin_w, pout_w = 1, pin, pout
    if row_bytes + 64 > WINDOW_ABOVE:
        rows_fit = BUDGET // (rs * 16)
        pout_w = ((rows_fit - kw) // stride + 1) & ~15
        assert pout_w >= 16
        nwin = (pout + pout_w - 1) // pout_w
        pin_w = (pout_w - 1) * stride + kw
        cb = 1
    plane = (cb * pin_w * rs + 63) & ~63
    return ConvPlan(nw, (oc // 16) % nw != 0, cb, nwin, pin_w, pout_w, pout - (nwin - 1) * pout_w, rs, plane * 16 + 64)


def ntv_of(ncols):
    """The NTV of the conv_stream_item / conv16_item forms that an iteration of `ncols` columns runs."""
    ntiles = (ncols + 15) // 16
    return ({CONV_NT} if ntiles >= CONV_NT else set()) | ({ntiles % CONV_NT} if ntiles % CONV_NT else set())


def conv_iterations(plan, pout, n):
    """(iterations of the launch, column counts that occur in them) for n chunks."""
    if plan.nwin > 1:
        return n * plan.nwin, {plan.pout_w, plan.last_cols}
    cols = ({plan.cb * pout} if n >= plan.cb else set()) | ({n % plan.cb * pout} if n % plan.cb else set())
    return (n + plan.cb - 1) // plan.cb, cols


def conv_ntv(plan, pout, n):
    return set().union(*(ntv_of(c) for c in conv_iterations(plan, pout, n)[1]))


LstmPlan = namedtuple("LstmPlan", "nt threads lds")


def lstm_stream_plan(size):
    """launch_lstm_stream (k_stream.hip): 16 NT chunks per group on 4 H threads, two x and two h images of four planes."""
    nt = 4 if size <= 128 else 2
    rs = size // 4 + 4 if (size // 16) % 2 == 0 else size // 4
    return LstmPlan(nt, 4 * size, 4 * 4 * 16 * nt * rs * 4)


def lstm_stream16_plan(size):
    """launch_lstm_stream16 (k_stream16.hip): rows of 2 H + 16 bytes, two x and two h images."""
    nt = 4 if size <= 128 else 2
    return LstmPlan(nt, 4 * size, 4 * 16 * nt * (2 * size + 16))


Conv16Plan = namedtuple("Conv16Plan", "nw cb lds")


def conv16_plan(ic, oc, kw, pin, pout, n, cus):
    """launch_conv16_t (k_stream16.hip) for a sub-batch of n chunks on `cus` CUs: cb is halved until every CU has an iteration;
    lds above LDS_LIMIT is the launcher's refusal ("chunk contexts this long run in fp32 ...")."""
    rb = 2 * ic + 16
    cb = _best_cb(max(1, min(8, BUDGET // (pin * rb))), pout)
    while cb > 1 and (n + cb - 1) // cb < cus:
        cb = (cb + 1) // 2
    return Conv16Plan(waves(oc), cb, (cb * pin + kw + 2) * rb)


# ---- fp32 cases: (group, size, L, batch sizes, the path the case is there for) ----------------------------------------------------
Case = namedtuple("Case", "group size L batches path")
SIZES = tuple(range(80, 257, 16))
NEW_WIDTHS = (144, 160, 192, 208, 224, 240)                       # never run before (ConvLSTM_w_ref, fp32)
STEP_SIZES, STEP_LENGTHS = (80, 128, 144, 208, 256), (29, 32, 35)  # T = 1, 2, 3
N, N_BIG = 37, 1024 + 37
WINDOW_SWITCH = ((256, 230, False), (256, 233, True), (224, 260, False), (224, 263, True), (128, 437, False), (128, 440, True))
MANY_WINDOWS = 260   # chunks of (256, 233): 1300 window iterations, more than the 4 x CUs blocks of a GPU of up to 324 CUs (an MI355X: 1024)
SUB_BATCHES = ((0, 1), (5, 3), (7, 15), (100, 16), (300, 17))


def _fp32_cases():
    out = []
    for size in SIZES:
        nt = lstm_stream_plan(size).nt
        out.append(Case("widths", size, 100, (N, 16 * nt + 1), f"nw {waves(size)}, lstm NT {nt}: one group and one chunk more"))
    for size in STEP_SIZES:
        for L in STEP_LENGTHS:
            out.append(Case("steps", size, L, (N, N_BIG), f"T {layer_rows(L)[3]}: merge_conv1 one ragged tile, cb 4..8; sig_conv3 2 / 3 / 4 tiles"))
    for size, L, win in WINDOW_SWITCH:
        out.append(Case("window", size, L, (5,), "windows, the last partial" if win else "no windows: the largest image"))
    out.append(Case("window", 256, 233, (MANY_WINDOWS,), "1300 window iterations: the first of 4 x CUs blocks take a second one and restage"))
    out.append(Case("remainder", 256, 266, (5,), "five full windows of 16 columns"))
    out.append(Case("remainder", 256, 269, (5,), "a sixth window of one column (rows == KW)"))
    out.append(Case("trips", 80, 32, (65536 + N,), "NT 4: a second group for 37 chunks' blocks"))
    out.append(Case("trips", 144, 32, (32768 + N,), "NT 2: a second group, against a reference"))
    return tuple(out)


FP32_CASES = _fp32_cases()
LONG_CASES = tuple(c for c in FP32_CASES if c.group in ("window", "remainder") and c.batches == (5,))
# what the teeth check of tests/test_host_stream_cases.py perturbs: (chunk of the five, 16-channel tile of merge_conv1's output)
TEETH_CHUNK, TEETH_TILE = 0, 2


def weights_seed(size):
    """synth_state's seed of every fp32 case.  Not `size` itself: with seed = size and the five synth_chunks of the long cases no
    (chunk, tile) passes the teeth check at all three positions (the best, chunk 3 tile 7, moves the logits of (128, 437) by
    2.8e-4 from position T / 2); of size + 1000 k, k = 1 .. 4, this one gives the largest smallest move (7.0e-4)."""
    return size + 4000

# ---- 16-bit cases (both dtypes each): (group, size, L, chunks; None: 8 x CUs + 37) -------------------------------------------------
Case16 = namedtuple("Case16", "group size L n path")
DTYPES16 = ("bf16", "f16")
N16, N16_STEPS = 1500, 1061
CASES16 = (tuple(Case16("widths16", size, 100, N16, f"nw {waves(size)}, NT 2") for size in (192, 224)) +
           tuple(Case16("steps16", size, L, N16_STEPS, f"T {layer_rows(L)[3]}") for size in (96, 256) for L in STEP_LENGTHS) +
           (Case16("cb8", 96, 100, None, "sig_conv3 keeps cb 8"),))
LDS_EDGE16 = (256, 464, 467)  # size, the longest chunk merge_conv1 stages (150 rows, 163 280 B), the first one refused
