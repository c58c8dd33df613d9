"""The case tables of tests/test_gpu_data_kernels.py, launch_encode's choice of kernel restated, and plain numpy restatements
of what the chunk data kernels of remora_amd/csrc/k_data.hip compute.

encode_kernel<PF, NST> has two forms of producing a chunk's floats.  The general form selects per element and is right for any
shape.  The code form loads four positions of one output row at once and packs a k-mer three bits per base into 32 bits: it is
right only for chunk lengths that are multiples of 4 and k-mers of up to 10 bases.  NST > 0 (the store loop unrolled for the
shipped shapes) runs the code form whatever the shape, so launch_encode has to hand only valid shapes to those instantiations.
encode_plan restates that choice for the rule as it was ("nst": by the store count alone) and as it is ("fixed"), so that
tests/test_host_data_cases.py can assert without a GPU which path every case takes, that the old rule sent shapes to a kernel
that is wrong for them, and that the present one sends none.

The numpy restatements (tally_ref, count_ref, trim_ref, motif_flags_ref) are what the GPU tests hold the kernels to; the host
tests hold THEM to the oracle, np.argmax, a float64 cross entropy and Motif.findall first.

A plain module (no tests in it), like stream_cases.py."""
from collections import namedtuple

import numpy as np

# ---- launch_encode, restated -------------------------------------------------------------------------------------------------------
ENCODE_LDS_LIMIT = 64 * 1024       # the default dynamic-LDS limit of a launch: launch_encode refuses what needs more
ENCODE_MAX_FLOATS = 1 << 21        # 4 K L at or above this: "chunk too large"
UNROLLED_NST = (15, 29, 10, 19)    # the store counts of the shipped shapes, in the order launch_encode tests them
SHIPPED = ((9, 100), (9, 200), (6, 100), (6, 200))

EncodePlan = namedtuple("EncodePlan", "pf nst NST code_form valid lds")


def pad16(x):
    return (x + 15) & ~15


def encode_plan(K, L, seq_w, map_w, form=2, rule="fixed"):
    """launch_encode (k_data.hip) for k-mers of K bases, chunks of L samples and rows of seq_w / map_w elements under
    RMR_ENCODE_FORM = form.  pf: row elements a lane prefetches (0: rows read where needed); nst: 16-byte stores per lane and
    chunk; NST: the instantiation's unrolled store count (0: the plain loop); code_form: what the kernel then runs; valid: the
    code form, when run, is right for the shape; lds: bytes of the launch."""
    wide = max(seq_w, map_w)
    pf = (1 if wide <= 64 else 2 if wide <= 128 else 4 if wide <= 256 else 0) if form >= 1 else 0
    nst = (K * L + 63) // 64
    code_ok = L % 4 == 0 and K <= 10
    unrolled = pf == 1 and form >= 2 and nst in UNROLLED_NST and (rule == "nst" or code_ok)
    assert rule in ("nst", "fixed")
    NST = nst if unrolled else 0
    code_form = NST > 0 or code_ok
    Lp = (L + 7) & ~7
    mapb = pad16(map_w * 2) if pf else 0
    per_wave = pad16(Lp * 4 + pad16(seq_w) + mapb)
    return EncodePlan(pf, nst, NST, code_form, code_ok or not code_form, 4 * per_wave)


def colliding_pairs(rule, nst, k_max=21, l_min=4, l_max=256, width=64):
    """(K, L) that `rule` sends to the unrolled kernel of `nst` stores although the code form is wrong for them (rows of
    `width` elements: prefetched one per lane, as the unrolled kernels need)."""
    return [(K, L) for K in range(1, k_max + 1) for L in range(l_min, l_max + 1)
            for p in [encode_plan(K, L, width, width, 2, rule)] if p.NST == nst and not p.valid]


# ---- encode cases ------------------------------------------------------------------------------------------------------------------
# name, kb, ka, L, longest chunk (bases), the path the case is there for:
#   unrolled<nst>  an unrolled instantiation, code form (valid)
#   collide<nst>   the old rule took the unrolled kernel of <nst> stores; now the plain loop in the general form
#   code           plain loop, code form
#   general        plain loop, general form
EncodeCase = namedtuple("EncodeCase", "name kb ka L max_len path")
N_SWEEP = 37   # nine blocks of four waves and one wave more


def _encode_cases():
    out = [EncodeCase(f"shipped-{kb + ka + 1}x{L}", kb, ka, L, 20, f"unrolled{(kb + ka + 1) * L // 64 + 1}")
           for kb, ka, L in ((4, 4, 100), (4, 4, 200), (2, 3, 100), (2, 3, 200))]
    # other shapes the unrolled kernels are right for: slot 9 of the code in use; a last store round of 24 lanes; full last rounds
    out += [EncodeCase(f"unrolled-{kb + ka + 1}x{L}", kb, ka, L, 20, f"unrolled{nst}")
            for kb, ka, L, nst in ((5, 4, 96, 15), (2, 2, 120, 10), (3, 4, 152, 19), (4, 3, 232, 29))]
    collide = {15: ((2, 3, 150), (4, 5, 90), (5, 6, 75), (7, 7, 60), (4, 4, 101)),   # L % 4 == 2 twice, K 12 odd L, K 15, odd L
               29: ((4, 4, 202), (4, 4, 201), (6, 5, 152), (2, 3, 301)),             # L % 4 == 2, odd, K 12 at L % 4 == 0, odd
               10: ((2, 3, 101), (3, 2, 102), (5, 5, 56), (1, 1, 202)),              # odd, L % 4 == 2, K 11, K 3
               19: ((2, 3, 201), (3, 2, 202), (6, 5, 100))}                          # odd, L % 4 == 2, K 12
    for nst, shapes in collide.items():
        out += [EncodeCase(f"collide{nst}-{kb + ka + 1}x{L}", kb, ka, L, 20, f"collide{nst}") for kb, ka, L in shapes]
    out += [EncodeCase("k10-code-limit", 4, 5, 40, 20, "code"), EncodeCase("k11-past-code-limit", 5, 5, 40, 20, "general"),
            EncodeCase("k1", 0, 0, 36, 20, "code"), EncodeCase("k21", 10, 10, 33, 30, "general"),
            EncodeCase("L4", 2, 0, 4, 6, "code"), EncodeCase("L5", 2, 0, 5, 6, "general"), EncodeCase("L7", 0, 2, 7, 6, "general"),
            EncodeCase("L8", 1, 1, 8, 6, "code"), EncodeCase("L94-pad2", 1, 2, 94, 20, "general"),
            EncodeCase("L1000", 1, 0, 1000, 40, "code"),
            EncodeCase("lds-limit", 0, 0, 4088, 7, "code")]   # 4 (4088 x 4 + 16 + 16) = 65536 bytes: the most that is launched
    return tuple(out)


ENCODE_CASES = _encode_cases()
HOST_FORM_CASES = ("shipped-9x100", "collide15-6x150", "collide29-12x152", "k21", "L5", "L1000")  # also through RMR_MEM_HOST
ENCODE_REFUSED = (0, 0, 4089, 7)      # kb, ka, L, longest chunk: one padded row of 4096 positions more than fits
WIDTHS = (64, 65, 128, 129, 256, 257)  # array widths either side of every prefetch step
WIDTH_SHAPES = {64: (1, 1, 36), 65: (2, 0, 36), 128: (1, 1, 34), 129: (0, 2, 36), 256: (1, 1, 35), 257: (1, 1, 36)}  # kb, ka, L


def second_trip_chunks(cus):
    """Chunks of a launch whose every wave gets a second chunk (grid 8 x CUs blocks of four waves) and five more."""
    return 4 * 8 * cus + 5


def encode_inputs(kb, ka, L, n, max_len, seq_w=None, map_w=None, seed=0):
    """(seqs int8 [n][seq_w], maps int16 [n][map_w], lens int16 [n]) of n chunks of L samples: lengths uniform in 1 .. max_len
    with chunks 1, 2 and 3 of 0, 1 and max_len bases (chunk 0 fixes the chunk length: maps[0][lens[0]]); mapping rows
    non-decreasing (bases without samples among them), ends forced to 0 and L as chunk extraction writes them; 6 % of the
    context's bases -1; beyond a chunk's own entries both rows hold arbitrary values (nothing may read them)."""
    rng = np.random.default_rng([seed, kb, ka, L, n])
    K = kb + ka + 1
    seq_w = max_len + K - 1 if seq_w is None else seq_w
    map_w = max_len + 1 if map_w is None else map_w
    assert seq_w >= max_len + K - 1 and map_w >= max_len + 1 and L < 32768
    lens = rng.integers(1, max_len + 1, n).astype(np.int16)
    for i, v in ((1, 0), (2, 1), (3, max_len)):
        if i < n:
            lens[i] = v
    maps = rng.integers(0, L + 1, (n, map_w)).astype(np.int16)
    seqs = rng.integers(-1, 4, (n, seq_w)).astype(np.int8)
    col = np.arange(map_w)[None, :]
    inner = np.sort(np.where(col <= lens[:, None], maps, np.int16(32767)), axis=1)
    maps = np.where(col <= lens[:, None], inner, maps)
    maps[:, 0] = 0
    maps[np.arange(n), lens] = L
    ctx = np.arange(seq_w)[None, :] < (lens[:, None] + K - 1)
    real = rng.integers(0, 4, (n, seq_w)).astype(np.int8)
    real[rng.random((n, seq_w)) < 0.06] = -1
    seqs = np.where(ctx, real, seqs)
    return np.ascontiguousarray(seqs), np.ascontiguousarray(maps), lens


def encode_ref(kb, ka, seqs, maps, lens):
    """compute_encoded_kmer_batch in numpy, by gathering: position s of a chunk belongs to the last base p with
    maps[p] <= s; out[c][4 kp + b][s] = 1 where that base exists and seqs[c][p + kp] == b."""
    n, K = lens.size, kb + ka + 1
    L = int(maps[0, lens[0]])
    out = np.zeros((n, 4 * K, L), np.float32)
    for c in range(n):
        sl = int(lens[c])
        p = np.searchsorted(maps[c, : sl + 1], np.arange(L), side="right") - 1
        ok = (p >= 0) & (p < sl)
        for kp in range(K):
            b = seqs[c, np.where(ok, p, 0) + kp].astype(np.int64)
            hit = ok & (b >= 0)
            out[c, 4 * kp + b[hit], np.flatnonzero(hit)] = 1.0
    return out


# ---- validation tally and label counts ---------------------------------------------------------------------------------------------
BLOCK = 256


def tally_sizes(cus):
    """Rows either side of a wave and of a block, and enough that blocks of the capped grid (4 x CUs) take a second trip."""
    return (1, 63, 64, 65, 255, 256, 257, 4 * cus * BLOCK + 257)


NUM_LABELS = (1, 2, 3, 5, 8, 15, 16)
COUNT_NUM_OUT = (1, 2, 3, 8, 16)


def label_maps(kf):
    """{form: label_of_column int32[kf]} - the model's column of every label, -1 where the model has none."""
    rng = np.random.default_rng(kf)
    forms = {"equal": np.arange(kf, dtype=np.int32), "permuted": rng.permutation(kf).astype(np.int32)}
    if kf >= 2:
        u = max(1, kf // 3)
        for name, first in (("front", 0), ("middle", (kf - u) // 2 if kf > 2 else 0), ("end", kf - u)):
            if name == "middle" and kf == 2:
                continue
            loc = np.full(kf, -1, np.int32)
            keep = [c for c in range(kf) if not first <= c < first + u]
            loc[keep] = np.arange(len(keep))
            forms[name] = loc
    return forms


def tally_logits(n, km, seed, special=True, nonfinite=False):
    """float32 [n][km] ~ N(0, 8^2); of every 16 rows (when `special`) one with its maximum twice or more (the first wins), one
    wholly below -1000 and one with an entry of exactly -1000 above the rest (a tie with an unmodelled column); with
    `nonfinite` three more hold NaN, +inf and -inf entries (first one each, then several kinds in a row)."""
    rng = np.random.default_rng([seed, n, km])
    x = (8.0 * rng.standard_normal((n, km))).astype(np.float32)
    r = np.arange(n)
    if special:
        tie = r[r % 16 == 3]
        x[tie] = np.round(x[tie])                         # few distinct values: ties of any multiplicity
        first = rng.integers(0, km, tie.size)
        x[tie, first] = 40.0
        x[tie, (first + rng.integers(1, max(km, 2), tie.size)) % km] = 40.0   # another column (km > 1)
        low = r[r % 16 == 7]
        x[low] = -2000.0 - np.abs(x[low])
        edge = r[r % 16 == 11]
        x[edge] = -2000.0 - np.abs(x[edge])
        x[edge, rng.integers(0, km, edge.size)] = -1000.0
    if nonfinite:
        for k, vals in ((1, (np.nan,)), (5, (np.inf,)), (9, (-np.inf,)), (13, (np.nan, np.inf, -np.inf, np.nan))):
            rows = r[r % 16 == k]
            for v in vals:
                x[rows, rng.integers(0, km, rows.size)] = v
        allneg = r[r % 32 == 15]
        x[allneg] = -np.inf
    return x


def widen(logits, kf, loc):
    """validate.add_unmodeled_labels as rmr_validation_tally takes it: column c of the result is the model's column loc[c],
    or -1000."""
    wide = np.full((logits.shape[0], kf), -1000.0, np.float32)
    for c in range(kf):
        if loc[c] >= 0:
            wide[:, c] = logits[:, loc[c]]
    return wide


TallyRef = namedtuple("TallyRef", "call confusion win32 win64 finite terms")


def tally_ref(logits, labels, kf, loc):
    """What rmr_validation_tally computes for one batch: the call (np.argmax of the widened logits: first maximum, first NaN),
    the confusion counts (true x called) by np.add.at, the called class's probability by the reference's float32 softmax
    (subtract the row maximum, exp, divide by the sum) and by a float64 one, which rows are finite throughout, and every
    row's cross entropy in float64 (log of the sum of exp, minus the label's logit)."""
    wide = widen(logits, kf, loc)
    call = np.argmax(wide, axis=1)
    conf = np.zeros((kf, kf), np.int64)
    np.add.at(conf, (labels, call), 1)
    rows = np.arange(wide.shape[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e32 = np.exp(wide - wide.max(axis=1, keepdims=True))
        s32 = np.zeros(wide.shape[0], np.float32)
        for c in range(kf):  # the sequential sum of a row, as the kernel and a plain loop add (np.sum adds in another order from 8 on)
            s32 = s32 + e32[:, c]
        win32 = e32[rows, call] / s32
        w64 = wide.astype(np.float64)
        mx = w64.max(axis=1, keepdims=True)
        e64 = np.exp(w64 - mx)
        win64 = e64[rows, call] / e64.sum(axis=1)
        terms = mx[:, 0] + np.log(e64.sum(axis=1)) - w64[rows, labels]
    return TallyRef(call.astype(np.uint8), conf, win32.astype(np.float32), win64, np.isfinite(wide).all(axis=1), terms)


def count_ref(logits, num_out):
    return np.bincount(np.argmax(logits, axis=1), minlength=num_out).astype(np.int64)


# ---- trim --------------------------------------------------------------------------------------------------------------------------
# stored context, kept context: (stored_before > cc_before, stored_after > cc_after) in its four combinations
TRIM_CONTEXTS = (((60, 70), (40, 45)), ((60, 70), (60, 45)), ((60, 70), (40, 70)), ((60, 70), (60, 70)))
TRIM_SIZES = (255, 256, 257)
TRIM_SEQ_CONTEXT = 5   # kb + ka of the stored dataset


def trim_inputs(stored, kept, n, max_len=24, seed=0):
    """A stored dataset's (seqs, maps, lens) with the mapping already shifted by the start difference, as the caller of
    trim_sb_chunk_context_core hands it over.  Of every 8 chunks one has every base but the last left of the kept window,
    one every entry but the first at or beyond the kept width, one a single base."""
    rng = np.random.default_rng([seed, n, *stored, *kept])
    (sb, sa), (cb, ca) = stored, kept
    Ls = sb + sa
    lens = rng.integers(1, max_len + 1, n).astype(np.int16)
    lens[np.arange(n) % 8 == 5] = 1
    col = np.arange(max_len + 1)[None, :]
    lo, hi = np.zeros((n, 1), np.int64), np.full((n, 1), Ls + 1, np.int64)
    hi[np.arange(n) % 8 == 1] = sb - cb + 1          # interior entries <= sb - cb: not right of the window's first sample
    lo[np.arange(n) % 8 == 3] = min(sb + ca, Ls)     # interior entries at or beyond the kept width
    maps = np.sort(np.where(col <= lens[:, None], rng.integers(lo, hi, (n, max_len + 1)), 32767), axis=1)
    maps[:, 0] = 0
    maps[np.arange(n), lens] = Ls
    maps = np.where(col <= lens[:, None], maps - (sb - cb), 0).astype(np.int16)
    seq_w = max_len + TRIM_SEQ_CONTEXT
    seqs = rng.integers(0, 4, (n, seq_w)).astype(np.int8)
    seqs[np.arange(seq_w)[None, :] >= lens[:, None] + TRIM_SEQ_CONTEXT] = -1
    return seqs, maps, lens


def trim_ref(stored, kept, tsc, seqs, maps, lens):
    """trim_sb_chunk_context_core on copies, in plain Python, as the reference's loops run - and asserting that every index
    those loops touch lies inside its row: the reference (and the oracle) have no guards, the inputs must not need any."""
    (sb, sa), (cb, ca) = stored, kept
    seqs, maps, lens = seqs.copy(), maps.copy(), lens.copy()
    n, map_w = maps.shape
    seq_w, width = seqs.shape[1], cb + ca
    for c in range(n):
        cm, cs, sl = maps[c], seqs[c], int(lens[c])
        if sb > cb:
            clip = 0
            while True:
                assert clip + 1 < map_w
                if cm[clip + 1] > 0:
                    break
                clip += 1
            assert sl + tsc <= seq_w and clip <= sl
            cm[: sl + 1 - clip] = cm[clip : sl + 1].copy()
            cs[: sl + tsc - clip] = cs[clip : sl + tsc].copy()
            sl -= clip
            cm[0] = 0
        if sa > ca:
            while True:
                assert sl - 1 >= 0
                if cm[sl - 1] < width:
                    break
                sl -= 1
            assert 1 <= sl < map_w
            cm[sl] = width
        lens[c] = sl
    return seqs, maps, lens


# ---- motif flags -------------------------------------------------------------------------------------------------------------------
# read lengths: read boundaries at bases 15, 16, 17, 4095, 4096 and 4097 of the concatenation (a thread takes 16 bases, a block
# 4096); empty reads first, in the middle (two) and last; 4807 bases in all: a last thread of 7
MOTIF_READ_LENGTHS = (0, 15, 1, 1, 0, 0, 4078, 1, 1, 710, 0)
MOTIF_SETS = {"len16": (("ANNNNNNNNNNNNNNC", 7),),
              "eight": (("CG", 0), ("DRACH", 2), ("GATC", 1), ("CCWGG", 1), ("TNA", 1), ("GC", 1), ("AAT", 0), ("RGY", 2)),
              "negative-focus": (("NNCG", 0),),      # normalised to CG with focus -2
              "iupac-n": (("TNA", 1),)}
# (motif, base): the motif lies over a read boundary there - the base is flagged in the concatenation read as ONE read, in no read of its own
STRADDLES = ((("ANNNNNNNNNNNNNNC", 7), 7), (("CG", 0), 4094), (("NNCG", 0), 4092), (("GC", 1), 4096))


def motif_reads(seed=0):
    """The reads of MOTIF_READ_LENGTHS (2 % of the bases -1), with a CG, a GC and an A .. C sixteen bases long laid over read
    boundaries (STRADDLES)."""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(0, 4, k).astype(np.int8) for k in MOTIF_READ_LENGTHS]
    for r in reads:
        r[rng.random(r.size) < 0.02] = -1
    reads[6][-1], reads[7][0], reads[8][0] = 1, 2, 1       # C | G | C, one read each, at bases 4094 | 4095 | 4096
    reads[1][:] = np.where(reads[1] < 0, 0, reads[1])      # read 1 (bases 0 .. 14) and read 2 (base 15): A + 14 + C
    reads[1][0], reads[2][0] = 0, 1
    return reads


def concat_reads(reads):
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.int64)
    return np.concatenate(reads).astype(np.int8), off


def motif_flags_ref(reads, motifs):
    """flags uint8 [bases of all reads]: 1 where a motif hit of the base's OWN read has its focus on the base."""
    from remora_amd.util import Motif

    seq, off = concat_reads(reads)
    want = np.zeros(seq.size, np.uint8)
    for r, o in zip(reads, off):
        for raw, focus in motifs:
            mot = Motif(raw, focus)
            fb = mot.findall(r.astype(np.int64)) + mot.focus_pos
            want[o + fb[(fb >= 0) & (fb < r.size)]] = 1
    return want


def motif_set(motifs):
    """rmr_motif_set of a motif list, as DeviceReads.motif_focus_bases fills it."""
    from remora_amd import _lib as L
    from remora_amd.util import Motif

    ms = L.MotifSet()
    ms.n_motifs = len(motifs)
    for m, (raw, focus) in enumerate(motifs):
        mot = Motif(raw, focus)
        ms.len[m], ms.focus_pos[m] = len(mot.raw_motif), int(mot.focus_pos)
        for k, allowed in enumerate(mot.int_pattern):
            ms.mask[m][k] = int(sum(1 << int(b) for b in allowed))
    return ms


# ---- extraction --------------------------------------------------------------------------------------------------------------------
EXTRACT_CONTEXT, EXTRACT_KMER = (13, 28), (2, 5)
# (signal samples, bases, focus bases or None): signal lengths 1, 7, 8, 9, 2049 - groups of eight samples cross reads and end inside
# them; reads without focus bases first, in the middle (two) and last; a read of one base; focus on first and last bases
EXTRACT_READS = ((9, 3, None), (7, 2, (0, 1)), (1, 1, (0,)), (8, 4, (0, 3)), (1, 1, None), (2049, 200, None), (2049, 180, (0, 57, 58, 179)),
                 (9, 9, (0, 8)), (7, 1, (0,)), (8, 5, None))


def extract_reads(seed=0):
    """[dict(dacs, shift, scale, seq_to_sig_map, int_seq, focus_bases)] of EXTRACT_READS: every base one sample or more."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (n_sig, nb, focus) in enumerate(EXTRACT_READS):
        cuts = np.sort(rng.choice(np.arange(1, n_sig), nb - 1, replace=False)) if nb > 1 else np.zeros(0, np.int64)
        s2s = np.concatenate([[0], cuts, [n_sig]]).astype(np.int64)
        out.append(dict(dacs=rng.integers(300, 701, n_sig).astype(np.int16), shift=480.0 + 3 * i, scale=75.0 - i, seq_to_sig_map=s2s,
                        int_seq=rng.integers(0, 4, nb).astype(np.int64), focus_bases=None if focus is None else np.array(focus, np.int64)))
    return out
