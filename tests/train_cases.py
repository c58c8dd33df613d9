"""The case table of tests/test_gpu_train_shapes.py and the launch arithmetic of the training step, restated.

One rmr_trainer_forward_backward is a fixed list of launches (api_train.hip) of the kernels of k_train.hip.  What a launch
looks like - the rows, K and columns of every matrix product, the grid of train_gemm_kernel, the slices of train_wgrad and how
the partials workspace (sized for max_batch at rmr_trainer_create) caps them, the blocks of a column sum, the grid of an LSTM
step - is decided on the host.  The functions below restate that arithmetic, so that tests/test_host_train_cases.py can assert
without a GPU that every case takes the path it is there for.  THE RESTATEMENT HAS TO FOLLOW THE KERNELS: when the launch code
changes, change it here, and look at the case table again - a case may no longer reach its path.

A plain module (no tests in it, no GPU import), like stream_cases.py."""
from collections import namedtuple

# ---- layer geometry (add_conv: Lout = (Lin - KW) / stride + 1) ---------------------------------------------------------------
Geometry = namedtuple("Geometry", "P1 P2 P3 T")


def geometry(L):
    """Rows per chunk of sig_conv1 / seq_conv1 (P1), sig_conv2 (P2), sig_conv3 / seq_conv2 (P3) and merge_conv1 = LSTM steps (T)."""
    P1 = (L - 5) + 1
    P2 = (P1 - 5) + 1
    P3 = (P2 - 9) // 3 + 1
    assert (P1 - 13) // 3 + 1 == P3  # rmr_trainer_create refuses a length at which the two branches disagree
    return Geometry(P1, P2, P3, (P3 - 5) + 1)


def conv_layers(size, L, K):
    """{layer: (IC, OC, KW, stride, Lin, Lout)} in the order of rmr_trainer_create's `layers`."""
    g = geometry(L)
    return {"sig_conv1": (1, 4, 5, 1, L, g.P1), "sig_conv2": (4, 16, 5, 1, g.P1, g.P2), "sig_conv3": (16, size, 9, 3, g.P2, g.P3),
            "seq_conv1": (4 * K, 16, 5, 1, L, g.P1), "seq_conv2": (16, size, 13, 3, g.P1, g.P3),
            "merge_conv1": (2 * size, size, 5, 1, g.P3, g.T)}


# ---- the products ---------------------------------------------------------------------------------------------------------------
Product = namedtuple("Product", "name R K NC")


def gemm_products(size, L, n, K, num_out):
    """Every train_gemm of one step: the forward convolutions but sig_conv1 (K = KW IC), the input halves of both LSTMs, the two
    products back through the LSTMs' input weights, and the data gradients (rows of stride x IC columns, K = J OC)."""
    g, S, out = geometry(L), size, []
    layers = conv_layers(size, L, K)
    for name in ("sig_conv2", "sig_conv3", "seq_conv1", "seq_conv2", "merge_conv1"):
        ic, oc, kw, st, lin, lout = layers[name]
        out.append(Product(name, n * lout, kw * ic, oc))
    out.append(Product("lstm1.in", n * g.T, S, 4 * S))
    out.append(Product("lstm2.in", n, S, 4 * S))
    out.append(Product("lstm2.dz1", n, 4 * S, S))
    out.append(Product("lstm1.dx", n * g.T, 4 * S, S))
    for name in ("merge_conv1", "sig_conv3", "sig_conv2", "seq_conv2"):  # conv_backward of a layer with an input gradient
        ic, oc, kw, st, lin, lout = layers[name]
        rows, J = (lin + st - 1) // st, (kw + st - 1) // st
        out.append(Product(name + ".data", n * rows, J * oc, st * ic))
    return out


def gemm_grid(p):
    """train_gemm: 64 rows x 64 columns per block."""
    return ((p.R + 63) // 64, (p.NC + 63) // 64)


def wgrad_products(size, L, n, K, num_out):
    """Every train_wgrad of one step, in the order of forward_backward (api_train.hip)."""
    g, S = geometry(L), size
    layers = conv_layers(size, L, K)
    out = [Product("fc", n, S, num_out), Product("lstm2.weight_ih", n, S, 4 * S), Product("lstm1.weight_ih", n * g.T, S, 4 * S),
           Product("lstm1.weight_hh", n * (g.T - 1), S, 4 * S)]
    for name in ("merge_conv1", "sig_conv3", "sig_conv2", "sig_conv1", "seq_conv2", "seq_conv1"):
        ic, oc, kw, st, lin, lout = layers[name]
        out.append(Product(name, n * lout, kw * ic, oc))
    return out


def part_w_floats(size, L, K, num_out, max_batch):
    """rmr_trainer_create's part_for: the largest K x NC x min(64, ceil(R / 256)) over the six convolutions, the LSTM products
    (R = max_batch T) and fc, at max_batch chunks."""
    g, S, N = geometry(L), size, max_batch
    sized = [(kw * ic, oc, N * lout) for ic, oc, kw, st, lin, lout in conv_layers(size, L, K).values()]
    sized += [(S, 4 * S, N * g.T), (S, num_out, N)]
    return max(k * nc * max(1, min(64, (r + 255) // 256)) for k, nc, r in sized)


WgradPlan = namedtuple("WgradPlan", "want cap rows_per slices grid")


def wgrad_plan(p, part_floats):
    """train_wgrad (k_train.hip).  R == 0 (lstm1.weight_hh at T = 1): no product, the reduction writes zeros."""
    if p.R <= 0:
        return WgradPlan(0, part_floats // (p.K * p.NC), 0, 0, None)
    want = (p.R + 255) // 256
    cap = part_floats // (p.K * p.NC)
    assert cap >= 1
    used = min(want, cap)
    rows_per = (p.R + used - 1) // used
    rows_per = (rows_per + 3) // 4 * 4
    slices = (p.R + rows_per - 1) // rows_per
    assert slices * p.K * p.NC <= part_floats  # the partials stay inside the workspace
    return WgradPlan(want, cap, rows_per, slices, ((p.K + 63) // 64, (p.NC + 63) // 64, slices))


def colsum_blocks(R):
    """train_colsum_blocks."""
    return max(1, min(1024, (R + 511) // 512))


def colsum_plan(R):
    """(blocks, rows per block) of a column sum over R rows (train_colsum)."""
    nblk = colsum_blocks(R)
    return nblk, (R + nblk - 1) // nblk


def colsum_rows(size, L, n, K, num_out):
    """{what is summed: R} of every column sum of a step: the BatchNorm passes of the six layers (forward and backward), the
    LSTM bias gradients, fc.bias."""
    g = geometry(L)
    out = {name: n * spec[5] for name, spec in conv_layers(size, L, K).items()}
    out.update({"lstm1.bias": n * g.T, "lstm2.bias": n, "fc.bias": n})
    return out


def lstm_grid(size, n):
    """train_lstm_step / train_lstm_step_bwd: 64 chunks x 16 units per block."""
    return ((n + 63) // 64, size // 16)


# ---- the facts a case is named after ----------------------------------------------------------------------------------------------
# k_tail16, k_tail64, nc_tail64 and nc_below_16 speak of the products whose shape the case CHOOSES: seq_conv1's K = 20 kmer_len,
# the NC = size of the size-wide products and fc's NC = num_out.  (sig_conv2's K = 20 and sig_conv1's NC = 4 give every case,
# old or new, a K tail and a narrow column block; a flag that is true everywhere would name nothing.)
Facts = namedtuple("Facts", "T colsum_second_trip colsum_capped wgrad_capped wgrad_second_trip k_tail16 k_tail64 nc_tail64 "
                            "nc_below_16 rows_partial_tile capped_products")
FLAGS = ("colsum_second_trip", "colsum_capped", "wgrad_capped", "wgrad_second_trip", "k_tail16", "k_tail64", "nc_tail64", "nc_below_16",
         "rows_partial_tile")


def facts(size, L, n, K, num_out, max_batch=None):
    max_batch = n if max_batch is None else max_batch
    assert 2 <= n <= max_batch
    part = part_w_floats(size, L, K, num_out, max_batch)
    plans = {p.name: wgrad_plan(p, part) for p in wgrad_products(size, L, n, K, num_out)}
    rows = colsum_rows(size, L, n, K, num_out)
    capped = tuple(name for name, pl in plans.items() if pl.want > pl.cap)
    return Facts(
        T=geometry(L).T,
        colsum_second_trip=any(colsum_blocks(r) > 64 for r in rows.values()),          # train_colsum_final_kernel's b += 64
        colsum_capped=any((r + 511) // 512 > 1024 for r in rows.values()),             # more than 512 rows per block
        wgrad_capped=bool(capped),                                                      # the workspace shortens the slice count
        wgrad_second_trip=any(pl.slices > 64 for pl in plans.values()),                # train_wgrad_reduce_kernel's z += 64
        k_tail16=(20 * K) % 16 != 0,                                                    # train_gemm_kernel's k0 += 16 ends inside a step
        k_tail64=(20 * K) % 64 != 0,                                                    # train_wgrad_kernel's last 64-row block of K
        nc_tail64=size % 64 != 0,                                                       # the last 64-column block is partial
        nc_below_16=num_out < 16,                                                       # fc: not one full 16-column tile
        rows_partial_tile=n % 64 != 0,                                                  # gemm rows (R = n), the LSTM step's 64 chunks
        capped_products=capped)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# shape: (size, L, n, K, num_out, variant[, max_batch]) - what tests/test_gpu_train_grads.py's run_case takes, max_batch added
Case = namedtuple("Case", "group shape path")
SIZES = tuple(range(16, 257, 16))
KMER_LENGTHS = tuple(range(1, 22))
CLASS_COUNTS = tuple(range(2, 17))
LENGTHS = tuple(range(29, 44))
BATCH_EDGES = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129)
SECOND_TRIP = (16, 100, 700, 1, 2, "seeded")
# colsum_capped needs more than 1024 x 512 rows in sig_conv1.  The starting point, (16, 100, 5500, K = 1), is not conditioned well
# enough for the gradient gate's 2e-5 floor: torch fp32 is 1.1e-5 from float64 there (bound: 5e-6, test_host_train_cases.py),
# and 7.7e-6 .. 3.7e-5 over 44 other seeds and lengths 100 .. 200 - with labels drawn independently of the inputs the true
# gradient is sampling noise that shrinks with the batch while fp32's rounding does not, and T = 24 LSTM steps add to it.
# Replaced by the shortest run of steps that still has a recurrent product (L 32: T = 2) with as many chunks as the path needs,
# and labels that can be learnt ("centre": the sign of the chunk's centre sample): 4.4e-6 with 8 torch threads, 3.3e-6 with 16
CAPPED = (16, 32, 18800, 1, 2, "centre")
INSIDE = (64, 100, 37, 9, 2, "seeded", 300)   # a batch inside a larger workspace
INSIDE_FULL = (64, 100, 300, 9, 2, "seeded")  # the batch that fills it (history independence)
RESIDENCY = (64, 100, 37, 9, 2, "mask")
WIDEST = (256, 41, 18, 9, 2, "seeded")
# variants: "seeded" (make_inputs' labels), "mask" (test_gpu_train_grads': every third row leaves the loss), "absent2" (the two
# last classes never occur), "keep1" (the mask keeps row 3 alone), "drop1" (the mask drops row 3 alone), "centre" (label 1
# where the chunk's centre sample is positive)
VARIANTS = ("seeded", "mask", "absent2", "keep1", "drop1", "centre")


def _cases():
    out = []
    for size in SIZES:
        out.append(Case("sizes", (size, 41, 18, 9, 2, "seeded"), f"NC {size} and {4 * size}: {(4 * size + 63) // 64} column blocks of the LSTM products"))
    for k in KMER_LENGTHS:
        out.append(Case("kmers", (16, 35, 9, k, 2, "seeded"), f"seq_conv1 K {20 * k}: gemm tail {20 * k % 16}, wgrad tail {20 * k % 64}"))
    for o in CLASS_COUNTS:
        out.append(Case("classes", (16, 33, 21, 9, o, "seeded"), f"num_out {o}"))
    out.append(Case("classes", (16, 33, 21, 9, 16, "absent2"), "num_out 16, classes 14 and 15 never occur"))
    for L in LENGTHS:
        g = geometry(L)
        out.append(Case("lengths", (32, L, 7, 9, 2, "seeded"), f"T {g.T}; stride-3 remainders {(g.P2 - 9) % 3} (sig_conv3), {(g.P1 - 13) % 3} (seq_conv2)"))
    for n in BATCH_EDGES:
        out.append(Case("batches", (16, 35, n, 9, 2, "seeded"), f"n {n}: {n % 64} chunks in the last 64-row tile"))
    out.append(Case("reductions", SECOND_TRIP, "colsum_second_trip, wgrad_capped, wgrad_second_trip"))
    out.append(Case("reductions", CAPPED, "colsum_capped"))
    out.append(Case("inside", INSIDE, "37 chunks in a workspace of 300"))
    out.append(Case("masks", (16, 35, 17, 9, 2, "keep1"), "the mask keeps one row"))
    out.append(Case("masks", (16, 35, 17, 9, 2, "drop1"), "the mask drops one row"))
    return tuple(out)


CASES = _cases()
MASK_ROW = 3


def case_id(shape):
    return "s%d_l%d_n%d_k%d_o%d_%s" % tuple(shape[:6]) + ("_w%d" % shape[6] if len(shape) > 6 else "")


def shape_facts(shape):
    size, L, n, K, num_out = shape[:5]
    return facts(size, L, n, K, num_out, shape[6] if len(shape) > 6 else None)


STATE_SEED = 11  # Trainer(seed=...) of every case, as in test_gpu_train_grads.run_case


def case_state(shape):
    """The initial state of a case's trainer, drawn on the CPU: what Trainer(size, K, num_out, L, seed=STATE_SEED) starts from."""
    from remora_amd import nets

    return {k: v.clone() for k, v in nets.build(shape[0], shape[3], shape[4], seed=STATE_SEED).state_dict().items()}


# make_inputs' seed is 5, as in test_gpu_train_grads.run_case, but where torch fp32 itself misses the conditioning bound of
# tests/test_host_train_cases.py (5e-6) with it: kmer_len 16 gives 5.96e-6 (lstm2.bias_ih_l0) at seed 5 and 1.2e-6 at seed 6
INPUT_SEED = {(16, 35, 9, 16, 2, "seeded"): 6}


def case_inputs(shape):
    """(sigs, enc, labels, mask) of a case: test_gpu_train_grads.make_inputs at INPUT_SEED (5), then the variant."""
    import numpy as np

    from test_gpu_train_grads import make_inputs

    size, L, n, K, num_out, variant = shape[:6]
    assert variant in VARIANTS
    sigs, enc, labels = make_inputs(size, L, n, K, num_out, seed=INPUT_SEED.get(tuple(shape), 5))
    mask = None
    if variant == "absent2":
        labels = labels % (num_out - 2)
    elif variant == "centre":
        labels = (sigs[:, 0, L // 2] > 0).astype(np.int64)
    elif variant == "mask":
        mask = np.arange(n) % 3 != 1
    elif variant == "keep1":
        mask = np.arange(n) == MASK_ROW
    elif variant == "drop1":
        mask = np.arange(n) != MASK_ROW
    return sigs, enc, labels, mask
