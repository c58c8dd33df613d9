"""The simplex-to-duplex aligner on the GPU (rmr_duplex_align, csrc/k_duplex.hip) against the reference's seven known answers,
against the numpy restatement (tests/duplex_restate.py: exact equality, the rule among co-optimal paths included) and, on the
long fixture pairs, against properties that hold for any optimal path."""
import json
import os

import numpy as np
import pytest

import duplex_restate as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")
S = 512  # the kernel's strip height (RMR_DUPLEX_STRIP_ROWS)
SIZES = [1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3]
KINDS = ["mutated", "duplex_overhang", "simplex_overhang", "single_base", "n_run"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _random(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n else ""


def _mutate(rng, seq, p_err=0.05, p_indel=0.1):
    """The reference fuzz's mutation (tests/test_duplex.py:21-35): 5 % substitutions, 10 % indels."""
    out = []
    for base in seq:
        if rng.uniform() <= p_err:
            base = rng.choice(list("ACGT"))
        if rng.uniform() <= p_indel:
            if rng.uniform() > 0.5:
                out += [base, rng.choice(list("ACGT"))]
            continue
        out.append(base)
    return "".join(out)


def _fit(rng, seq, n):
    return seq[:n] if len(seq) >= n else seq + _random(rng, n - len(seq))


def _grid_pairs():
    """(simplex, duplex) for every simplex length x duplex length of SIZES, the input kinds dealt round, then the long indels."""
    rng = np.random.default_rng(20)
    pairs = []
    for a, n in enumerate(SIZES):
        for b, m in enumerate(SIZES):
            kind = KINDS[(a + 2 * b) % len(KINDS)]
            duplex = _random(rng, m)
            simplex = _fit(rng, _mutate(rng, duplex), n)
            if kind == "duplex_overhang" and m > 12:
                k = int(rng.integers(2, m // 4 + 1))
                duplex = ("T" * k + duplex + "T" * k)[:m] if m < 40 else "T" * k + duplex[k:m - k] + "T" * k
            elif kind == "simplex_overhang" and n > 12:
                k = int(rng.integers(2, n // 4 + 1))
                simplex = "T" * k + simplex[k:n - k] + "T" * k
            elif kind == "single_base":
                simplex, duplex = "A" * n, "A" * m
            elif kind == "n_run" and m > 8:
                k = int(rng.integers(1, m // 3 + 1))
                at = int(rng.integers(0, m - k + 1))
                duplex = duplex[:at] + "N" * k + duplex[at + k:]
                if n > 8:
                    simplex = simplex[:n // 2] + "N" * min(3, n - n // 2) + simplex[n // 2 + min(3, n - n // 2):]
            assert len(simplex) == n and len(duplex) == m
            pairs.append((simplex, duplex))
    base = _random(rng, 900)
    for gap in (70, S + 30):  # one indel longer than a wave's 64 columns / lanes, one longer than a strip
        ins = _random(rng, gap)
        pairs.append((base[:450] + ins + base[450:], base))  # insertion in the simplex
        pairs.append((base, base[:450] + ins + base[450:]))  # deletion from the simplex
        pairs.append((_mutate(rng, base[:300]) + ins + _mutate(rng, base[300:]), base))
    return pairs


def _as_dict(res, a):
    ops, lens = res.runs(a)
    return dict(status=int(res.status[a]), score=int(res.score[a]), end_row=int(res.end_row[a]), query_start=int(res.query_start[a]),
                ref_start=int(res.ref_start[a]), ref_end=int(res.ref_end[a]), ops=ops, lens=lens)


@pytest.fixture(scope="module")
def grid(torch_cuda):
    from remora_amd import duplex_utils as DU

    pairs = _grid_pairs()
    return pairs, DU.align_batch(pairs), [R.align(s, d) for s, d in pairs]  # ONE launch: small and large alignments share it


def test_known_answers(torch_cuda):
    from remora_amd import data_chunks as DC
    from remora_amd import duplex_utils as DU

    for c in json.load(open(os.path.join(GOLDEN, "duplex_known_answers.json"))):
        got = DU.map_simplex_to_duplex(simplex_seq=c["simplex"], duplex_seq=c["duplex"])
        assert got.trimmed_duplex_seq == c["trimmed_duplex_seq"] and got.duplex_offset == c["duplex_offset"]
        assert got.duplex_to_simplex_mapping.tolist() == c["duplex_to_simplex_mapping"]
        sig = DC.map_ref_to_signal(query_to_signal=np.arange(len(c["simplex"])), ref_to_query_knots=got.duplex_to_simplex_mapping)
        assert sig.tolist() == c["duplex_to_signal"]


def test_grid_equals_the_restatement(grid):
    from remora_amd import duplex_utils as DU

    pairs, res, want = grid
    assert res.n_groups == 1
    kinds = set()
    for a, ((simplex, duplex), w) in enumerate(zip(pairs, want)):
        g = _as_dict(res, a)
        where = f"alignment {a}: simplex {len(simplex)}, duplex {len(duplex)}"
        for k in ("status", "score", "end_row", "query_start", "ref_start", "ref_end"):
            assert g[k] == w[k], (where, k, g[k], w[k])
        assert g["ops"].tolist() == w["ops"].tolist() and g["lens"].tolist() == w["lens"].tolist(), where
        if w["status"] == R.ST_OK:
            got = DU.mapping_from_alignment(res.pairwise_alignment(a), duplex)
            assert got.duplex_to_simplex_mapping.tolist() == R.mapping(w).tolist(), where
            assert got.duplex_to_simplex_mapping.size == w["ref_end"] - w["ref_start"] + 1
            kinds.update(np.unique(w["ops"]).tolist())
    assert kinds == {0, 1, 2} and {w["status"] for w in want} >= {R.ST_OK}
    # the clean long indels are found whole (the mutated third case of each may prefer a free simplex prefix)
    long_gaps = [int(want[a]["lens"][want[a]["ops"] != 0].max()) for a in (-6, -5, -3, -2)]
    assert long_gaps == [70, 70, S + 30, S + 30], long_gaps


def test_budget_groups_give_the_same_bytes(grid):
    from remora_amd import duplex_utils as DU

    pairs, res, _ = grid
    biggest = max(DU.trace_bytes(len(s), len(d)) for s, d in pairs)
    small = DU.align_batch(pairs, trace_budget=2 * biggest)
    assert small.n_groups >= 3
    for k in ("status", "score", "end_row", "query_start", "ref_start", "ref_end", "n_runs"):
        assert np.array_equal(getattr(small, k), getattr(res, k)), k
    for a in range(len(pairs)):
        assert small.words[small.run_off[a]:small.run_off[a] + small.n_runs[a]].tobytes() == \
            res.words[res.run_off[a]:res.run_off[a] + res.n_runs[a]].tobytes()


def test_statuses_leave_the_rest_of_the_batch_alone(torch_cuda):
    from remora_amd import duplex_utils as DU

    rng = np.random.default_rng(3)
    d = _random(rng, 700)
    s = _mutate(rng, d)
    big_d = _random(rng, 1500)
    pairs = [(s, d), (_mutate(rng, big_d), big_d), ("ACGU", "ACGT"), ("", "ACGT"), ("ACGT", ""), ("ACGT", "ACGTRACGT"), (d, s)]
    res = DU.align_batch(pairs, trace_budget=DU.trace_bytes(len(s) + 200, len(d) + 200))
    assert res.status.tolist() == [DU.STATUS_OK, DU.STATUS_OVER_BUDGET, DU.STATUS_BAD_BASE, DU.STATUS_EMPTY, DU.STATUS_EMPTY,
                                   DU.STATUS_BAD_BASE, DU.STATUS_OK]
    assert not res.n_runs[1:6].any() and not res.score[1:6].any()
    for a in (0, 6):
        w, g = R.align(*pairs[a]), _as_dict(res, a)
        assert all(g[k] == w[k] for k in ("score", "end_row", "query_start", "ref_start", "ref_end"))
        assert g["ops"].tolist() == w["ops"].tolist() and g["lens"].tolist() == w["lens"].tolist()
    maps = DU.map_simplexes_to_duplexes(pairs[:3], trace_budget=DU.trace_bytes(len(s) + 200, len(d) + 200))
    assert isinstance(maps[0], DU.SimplexDuplexMapping) and maps[1] == "duplex alignment exceeds the trace budget" and isinstance(maps[2], str)
    with pytest.raises(RuntimeError, match="failed to find match operations in pairwise alignment"):
        DU.map_simplex_to_duplex(simplex_seq="A", duplex_seq="CCCCCCCC")


def fixture_alignments():
    """The four alignments duplex calling makes for the two pairs of the fixture files, as DuplexRead.from_reads_and_alignment
    orients them: [(pair length class, simplex_seq, duplex_seq)]."""
    from remora_amd import io as rio

    simplex = {r.query_name: (rio.revcomp(r.query_sequence) if r.is_reverse else r.query_sequence)
               for r in rio.iter_bam_records(os.path.join(DATA, "simplex_reads_mapped.bam"))}
    duplex = {}
    for r in rio.iter_bam_records(os.path.join(DATA, "duplex_reads_mapped.bam")):
        duplex.setdefault(r.query_name.split(";")[0], r)
    out = []
    for line in open(os.path.join(DATA, "duplex_pairs.txt")):
        t, c = line.split()
        rec = duplex[t]
        first, second = (c, t) if rec.is_reverse else (t, c)
        out.append((simplex[first], rec.query_sequence))
        out.append((simplex[second], rio.revcomp(rec.query_sequence)))
    return out


def test_fixture_pairs_have_valid_optimal_paths(torch_cuda, tmp_path):
    from remora_amd import duplex_utils as DU

    pairs = fixture_alignments()
    assert sorted(len(d) for _, d in pairs) == [7782, 7782, 24561, 24561]
    res = DU.align_batch(pairs)
    assert res.status.tolist() == [0, 0, 0, 0]
    short = [a for a, (_, d) in enumerate(pairs) if len(d) < 10000]  # the 7.8 kb pair: the optimum itself, from the C++ twin
    want = dict(zip(short, R.align_cpp([pairs[a] for a in short], R.build_cpp(tmp_path))))
    for a, (simplex, duplex) in enumerate(pairs):
        g = _as_dict(res, a)
        score, q_end = R.path_score(simplex, duplex, g)  # asserts that the path is monotone and consumes the trimmed ranges
        assert score == g["score"] and q_end == g["end_row"], (a, score, g["score"], q_end, g["end_row"])
        assert g["score"] > 4 * min(len(simplex), len(duplex))  # the two reads of a pair do align
        if a in want:
            assert (g["score"], g["end_row"]) == (want[a]["score"], want[a]["end_row"]), a
            # (and, under the project's tie rule, the same path)
            assert all(np.asarray(g[k]).tolist() == np.asarray(want[a][k]).tolist() for k in g), a
