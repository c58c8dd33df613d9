"""A restatement of the simplex-to-duplex alignment to hold the GPU kernel against (tests/test_host_duplex.py,
tests/test_gpu_duplex_align.py): Gotoh's three-state DP in numpy, vectorised over anti-diagonals, with the project's rule among
co-optimal paths.  It shares no code with csrc/k_duplex.hip and none of its schedule (no strips, no lanes).

  query = simplex (rows i = 1..n, free ends), ref = duplex (columns j = 1..m, consumed whole)
  H[i][0] = 0, H[0][j] = -(OPEN + EXTEND (j - 1));  E = deletion state (consumes the duplex), F = insertion state
  E[i][j] = max(H[i][j-1] - OPEN, E[i][j-1] - EXTEND),  F[i][j] = max(H[i-1][j] - OPEN, F[i-1][j] - EXTEND)
  H[i][j] = max(H[i-1][j-1] + s(q_i, r_j), E[i][j], F[i][j]);  score = max_i H[i][m]

Rule: the end row is the smallest i of maximal H[i][m]; H prefers the diagonal, then E, then F; a gap state returns to H as soon
as the scores allow (when the open score is no worse than the extension)."""
import numpy as np

MATCH, MISMATCH, N_BASE, N_N = 5, -4, -2, -1
OPEN, EXTEND = 10, 2
NEG = -(1 << 40)
OP_M, OP_I, OP_D = 0, 1, 2
ST_OK, ST_NO_MATCH, ST_BAD_BASE, ST_OVER_BUDGET, ST_EMPTY = range(5)
_CODE = np.full(256, 5, np.int64)
for _k, _c in enumerate("ACGTN"):
    _CODE[ord(_c)] = _k
# substitution scores over A C G T N
SUB = np.full((5, 5), MISMATCH, np.int64)
SUB[np.arange(4), np.arange(4)] = MATCH
SUB[4, :] = SUB[:, 4] = N_BASE
SUB[4, 4] = N_N


def encode(seq):
    return _CODE[np.frombuffer(seq.encode("ascii", "replace"), np.uint8)]


def fill(query, ref, keep_trace=True):
    """Last column H[0..n][m] and, if asked, the trace T[i][j] (bits 0-1: source of H, 0 diagonal / 1 E / 2 F; bit 2: E
    extends; bit 3: F extends)."""
    q, r = encode(query), encode(ref)
    n, m = q.size, r.size
    T = np.zeros((n + 1, m + 1), np.uint8) if keep_trace else None
    last = np.full(n + 1, NEG, np.int64)
    last[0] = -(OPEN + EXTEND * (m - 1))
    # diagonals d = i + j, arrays indexed by i; h1 / e1 / f1: diagonal d - 1, h2: diagonal d - 2
    h2 = np.full(n + 1, NEG, np.int64)
    h1 = np.full(n + 1, NEG, np.int64)
    e1 = np.full(n + 1, NEG, np.int64)
    f1 = np.full(n + 1, NEG, np.int64)
    h2[0] = 0  # d = 0
    h1[0] = -OPEN  # d = 1: H[0][1]
    if n >= 1:
        h1[1] = 0  # H[1][0]
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - m), min(n, d - 1)  # rows of the interior cells of this diagonal
        i = np.arange(lo, hi + 1)
        j = d - i
        eo, ee = h1[lo:hi + 1] - OPEN, e1[lo:hi + 1] - EXTEND
        fo, fe = h1[lo - 1:hi] - OPEN, f1[lo - 1:hi] - EXTEND
        e, f = np.maximum(eo, ee), np.maximum(fo, fe)
        dg = h2[lo - 1:hi] + SUB[q[i - 1], r[j - 1]]
        g = np.maximum(e, f)
        h = np.maximum(dg, g)
        if keep_trace:
            src = np.where(dg >= g, 0, np.where(e >= f, 1, 2))
            T[i, j] = src | ((ee > eo) << 2) | ((fe > fo) << 3)
        hn = np.full(n + 1, NEG, np.int64)
        en = np.full(n + 1, NEG, np.int64)
        fn = np.full(n + 1, NEG, np.int64)
        hn[lo:hi + 1], en[lo:hi + 1], fn[lo:hi + 1] = h, e, f
        if d <= m:
            hn[0] = -(OPEN + EXTEND * (d - 1))  # row 0
        if d <= n:
            hn[d] = 0  # column 0
        if hi >= d - m >= 1:
            last[d - m] = h[d - m - lo]
        h2, h1, e1, f1 = h1, hn, en, fn
    return last, T


def align(query, ref):
    """dict(status, score, end_row, query_start, ref_start, ref_end, ops, lens): the trimmed path as runs in alignment order."""
    zero = dict(score=0, end_row=0, query_start=0, ref_start=0, ref_end=0, ops=np.zeros(0, np.int64), lens=np.zeros(0, np.int64))
    if len(query) == 0 or len(ref) == 0:
        return dict(zero, status=ST_EMPTY)
    if (encode(query) > 4).any() or (encode(ref) > 4).any():
        return dict(zero, status=ST_BAD_BASE)
    n, m = len(query), len(ref)
    last, T = fill(query, ref)
    end_row = int(np.argmax(last))  # the first maximum
    score = int(last[end_row])
    i, j, state, path = end_row, m, 0, []
    while j > 0:
        if i == 0:
            path.extend([OP_D] * j)
            j = 0
            break
        t = int(T[i, j])
        if state == 0:
            state = t & 3
            if state == 0:
                path.append(OP_M)
                i, j = i - 1, j - 1
        elif state == 1:
            path.append(OP_D)
            state = 1 if t & 4 else 0
            j -= 1
        else:
            path.append(OP_I)
            state = 2 if t & 8 else 0
            i -= 1
    path = np.array(path[::-1], np.int64)
    is_m = np.nonzero(path == OP_M)[0]
    if not is_m.size:
        return dict(zero, status=ST_NO_MATCH)
    head, tail = path[:is_m[0]], path[is_m[-1] + 1:]
    kept = path[is_m[0]:is_m[-1] + 1]
    cut = np.nonzero(np.diff(kept))[0] + 1
    starts = np.concatenate([[0], cut])
    return dict(status=ST_OK, score=score, end_row=end_row, query_start=i + int((head == OP_I).sum()), ref_start=int((head == OP_D).sum()),
                ref_end=m - int((tail == OP_D).sum()), ops=kept[starts], lens=np.diff(np.concatenate([starts, [kept.size]])))


def best_score(query, ref):
    """The optimal score and its end row alone (no trace kept: for long pairs)."""
    last, _ = fill(query, ref, keep_trace=False)
    return int(last.max()), int(np.argmax(last))


def mapping(res):
    """duplex_to_simplex_mapping of an align() result: per trimmed duplex position 0..ref_end - ref_start its simplex
    coordinate, exact on matches, interpolated in float64 across gaps and truncated (np.interp over the knots of the match
    runs, as the reference's make_sequence_coordinate_mapping has it), plus query_start."""
    ops, lens = res["ops"], res["lens"]
    rk, qk, rp, qp = [0], [0], 0, 0
    for op, ln in zip(ops.tolist(), lens.tolist()):
        if op == OP_M:
            rk += [rp, rp + ln - 1]
            qk += [qp, qp + ln - 1]
            rp, qp = rp + ln, qp + ln
        elif op == OP_I:
            qp += ln
        else:
            rp += ln
    rk.append(rp)
    qk.append(qp)
    return np.interp(np.arange(rp + 1), rk, qk).astype(int) + res["query_start"]


def path_score(query, ref, res):
    """The score of the reported path recomputed along it in O(n + m): the penalised leading and trailing duplex bases, the
    substitutions of the match runs and the gaps between them.  Also checks that the path consumes exactly the trimmed
    ranges [query_start, end_row) and [ref_start, ref_end)."""
    q, r = encode(query), encode(ref)
    ops, lens = res["ops"], res["lens"]
    assert ops.size and ops[0] == OP_M and ops[-1] == OP_M and (lens > 0).all() and (np.diff(ops) != 0).all()
    qp, rp, s = res["query_start"], res["ref_start"], 0
    gap = lambda k: OPEN + EXTEND * (k - 1)  # noqa: E731
    if rp:
        s -= gap(rp)
    for op, ln in zip(ops.tolist(), lens.tolist()):
        if op == OP_M:
            s += int(SUB[q[qp:qp + ln], r[rp:rp + ln]].sum())
            qp, rp = qp + ln, rp + ln
        elif op == OP_I:
            s -= gap(ln)
            qp += ln
        else:
            s -= gap(ln)
            rp += ln
    assert rp == res["ref_end"] and 0 <= res["ref_start"] < res["ref_end"] <= r.size
    assert 0 <= res["query_start"] < qp <= q.size
    if r.size - rp:
        s -= gap(r.size - rp)
    return s, qp


# ---- the C++ twin (tests/c/duplex_restate.cpp) for pairs too long for numpy ----
def build_cpp(out_dir):
    """Compile the twin into `out_dir`; its path."""
    import os
    import shutil
    import subprocess

    exe = os.path.join(str(out_dir), "duplex_restate")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "duplex_restate.cpp")
    cc = subprocess.run([shutil.which("g++") or "c++", "-O3", "-std=c++17", "-Wall", src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    return exe


def align_cpp(pairs, exe, rate=None):
    """align() for every (query, ref) of `pairs` through the twin; `rate` (a list) receives its cell updates per second."""
    import re
    import subprocess

    zero = dict(score=0, end_row=0, query_start=0, ref_start=0, ref_end=0, ops=np.zeros(0, np.int64), lens=np.zeros(0, np.int64))
    live = [(q, r) for q, r in pairs if len(q) and len(r)]
    run = subprocess.run([exe], input="".join(f"{q} {r}\n" for q, r in live), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    if rate is not None:
        rate.append(float(re.search(r"= ([0-9.e+]+) cell updates/s", run.stderr).group(1)))
    lines, out = iter(run.stdout.splitlines()), []
    for q, r in pairs:
        if not (len(q) and len(r)):
            out.append(dict(zero, status=ST_EMPTY))
            continue
        f = next(lines).split()
        st, score, end_row, qs, rs, re_, n_runs = (int(x) for x in f[:7])
        runs = [tuple(int(x) for x in w.split(":")) for w in f[7:]]
        assert len(runs) == n_runs
        out.append(dict(status=st, score=score, end_row=end_row, query_start=qs, ref_start=rs, ref_end=re_,
                        ops=np.array([o for o, _ in runs], np.int64), lens=np.array([k for _, k in runs], np.int64)))
    return out
